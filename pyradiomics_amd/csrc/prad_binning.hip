// prad_binning.hip -- on-device discretisation behind the C ABI (include/pyradiomics_amd.h): ROI minimum / maximum, digitize
// against bin edges with the level counts, the fixed-bin-count route (bincount) with its queue of tickets, level counts.
// The only unit that includes kernels_binning.h.
#include "prad_runtime.h"
#include "kernels_binning.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

using namespace prad;

namespace {
template <typename T>
int launch_digitize(const T *image, const uint8_t *mask, long long n, const double *e_d, int nedges, int32_t *levels,
                    int *top, unsigned long long *counts_d, hipStream_t s) {
  // 4 workgroups per CU: every workgroup ends with global atomics on the same few words (its maximum, its nb counters), and
  // those serialise in L2 at ~25 ns each -- with 4096 workgroups they were half of the kernel (256^3 float64: 124 -> 57 us;
  // roi_minmax 59 -> 35 with 512 instead of 2048; profiles/r03_probes.md, section 10)
  static const int cap = getenv("PRAD_BIN_BLOCKS") ? atoi(getenv("PRAD_BIN_BLOCKS")) : 1024;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap));
  const size_t edge_b = sizeof(double) * (size_t)nedges, cnt_b = 4 * sizeof(unsigned) * ((size_t)nedges + 1);
  const bool lds_edges = edge_b <= 60 * 1024;
  // counts in LDS while edges + four private tables fit 64 KB (nedges <= 2 700), otherwise straight global atomics
  // (that many levels spread the atomics over as many addresses)
  const size_t cnt3_b = 256 * sizeof(unsigned) * ((size_t)nedges + 1);     // a table per thread
  const int counts = !counts_d ? 0 : (nedges <= 48 ? 3 : ((lds_edges && edge_b + cnt_b <= 64 * 1024) ? 1 : 2));
#define PRAD_DIG(LE, CN)                                                                                              \
  hipLaunchKernelGGL((digitize_kernel<T, LE, CN>), dim3(gx), dim3(256),                                               \
                     (LE ? edge_b : 0) + (CN == 1 ? cnt_b : (CN == 3 ? cnt3_b : 0)), s, image, mask, n, e_d, nedges, levels, top, counts_d)
  if (lds_edges) {
    if (counts == 0) PRAD_DIG(true, 0);
    else if (counts == 1) PRAD_DIG(true, 1);
    else if (counts == 3) PRAD_DIG(true, 3);
    else PRAD_DIG(true, 2);
  } else {
    if (counts == 0) PRAD_DIG(false, 0);
    else PRAD_DIG(false, 2);
  }
#undef PRAD_DIG
  return check_launch("digitize_kernel");
}
}  // namespace

extern "C" {

// ---- on-device discretisation ----------------------------------------------------------------
int prad_roi_minmax_dev(const void *image, int dtype, const uint8_t *mask, long long n, double *minmax, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!image || !mask || !minmax || n < 1) return fail(PRAD_E_ARG, "roi_minmax: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *keys = nullptr;
  PRAD_TRY(c.get<unsigned long long>("minmax_keys", 2, &keys));
  // (pinned staging: a copy from / to pageable memory goes through the runtime's bounce buffer and blocks the host)
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned("bin_pin", 4096, &pin));
  unsigned long long *init = (unsigned long long *)pin, *outk = init + 2;
  init[0] = ~0ull;
  init[1] = 0ull;
  PRAD_HIP(hipMemcpyAsync(keys, init, 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  static const int cap = getenv("PRAD_MINMAX_BLOCKS") ? atoi(getenv("PRAD_MINMAX_BLOCKS")) : 512;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap));
  switch (dtype) {
    case 0: hipLaunchKernelGGL(roi_minmax_kernel<float>, dim3(gx), dim3(256), 0, s, (const float *)image, mask, n, keys); break;
    case 1: hipLaunchKernelGGL(roi_minmax_kernel<double>, dim3(gx), dim3(256), 0, s, (const double *)image, mask, n, keys); break;
    case 2: hipLaunchKernelGGL(roi_minmax_kernel<int>, dim3(gx), dim3(256), 0, s, (const int *)image, mask, n, keys); break;
    case 3: hipLaunchKernelGGL(roi_minmax_kernel<short>, dim3(gx), dim3(256), 0, s, (const short *)image, mask, n, keys); break;
    default: return fail(PRAD_E_ARG, "roi_minmax: dtype %d", dtype);
  }
  PRAD_TRY(check_launch("roi_minmax_kernel"));
  PRAD_HIP(hipMemcpyAsync(outk, keys, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  if (outk[1] == 0ull) return fail(PRAD_E_ARG, "roi_minmax: empty ROI");
  minmax[0] = f64_unkey(outk[0]);
  minmax[1] = f64_unkey(outk[1]);
  return PRAD_OK;
}

int prad_digitize_counts_dev(const void *image, int dtype, const uint8_t *mask, long long n, const double *edges,
                             int nedges, int32_t *levels, int *max_level, long long *counts, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!image || !mask || !edges || !levels || n < 1 || nedges < 1) return fail(PRAD_E_ARG, "digitize: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  double *e_d = nullptr;
  int *top = nullptr;
  unsigned long long *cnt_d = nullptr;
  PRAD_TRY(c.get<double>("bin_edges", (size_t)nedges, &e_d));
  PRAD_TRY(c.get<int>("bin_top", 1, &top));
  // host <-> device traffic of this call through one pinned block: [edges (nedges doubles) | top (8 B) | counts]
  const size_t pin_bytes = sizeof(double) * ((size_t)nedges + 1) + sizeof(long long) * ((size_t)nedges + 2);
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned("digitize_pin", pin_bytes, &pin));
  double *e_h = (double *)pin;
  int *top_h = (int *)(e_h + nedges);
  long long *cnt_h = (long long *)(e_h + nedges + 1);
  memcpy(e_h, edges, sizeof(double) * nedges);
  PRAD_HIP(hipMemcpyAsync(e_d, e_h, sizeof(double) * nedges, hipMemcpyHostToDevice, s));
  if (counts) {
    // counts and the level maximum sit in ONE device block [top | counts]: one memset, one copy back
    PRAD_TRY(c.get<unsigned long long>("bin_counts", (size_t)nedges + 2, &cnt_d));
    PRAD_HIP(hipMemsetAsync(cnt_d, 0, sizeof(unsigned long long) * ((size_t)nedges + 2), s));
    top = (int *)cnt_d;
    cnt_d += 1;
  } else {
    PRAD_HIP(hipMemsetAsync(top, 0, sizeof(int), s));
  }
  switch (dtype) {
    case 0: PRAD_TRY(launch_digitize((const float *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    case 1: PRAD_TRY(launch_digitize((const double *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    case 2: PRAD_TRY(launch_digitize((const int *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    case 3: PRAD_TRY(launch_digitize((const short *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    default: return fail(PRAD_E_ARG, "digitize: dtype %d", dtype);
  }
  if (counts) {
    PRAD_HIP(hipMemcpyAsync(top_h, cnt_d - 1, sizeof(long long) * ((size_t)nedges + 2), hipMemcpyDeviceToHost, s));   // [top | counts]
  } else {
    PRAD_HIP(hipMemcpyAsync(top_h, top, sizeof(int), hipMemcpyDeviceToHost, s));
  }
  PRAD_HIP(hipStreamSynchronize(s));
  if (max_level) *max_level = *top_h;
  if (counts) memcpy(counts, cnt_h, sizeof(long long) * ((size_t)nedges + 1));
  return PRAD_OK;
}

// the queueing half of prad_bincount_dev: slot in [0, PRAD_BIN_SLOTS) names the device block, the pinned block and the event
namespace {
constexpr int PRAD_BIN_SLOTS = 4;
struct BinSlots {
  int device = -1;
  hipEvent_t done[PRAD_BIN_SLOTS] = {};
  int nedges[PRAD_BIN_SLOTS] = {};
  unsigned long long *host[PRAD_BIN_SLOTS] = {};
  bool used[PRAD_BIN_SLOTS] = {};
  unsigned seq = 0;
};
BinSlots &bin_slots() {
  static thread_local BinSlots b;
  return b;
}
int bincount_queue(Context &c, int slot, const void *image, int dtype, const uint8_t *mask, long long n, int binCount, int32_t *levels,
                   hipStream_t s, unsigned long long **host_out) {
  const int nedges = binCount + 1;
  // one device block: [keys (2 u64) | info (8 B) | top (8 B) | counts (nedges + 1) | edges (nedges doubles)] -- one copy back
  unsigned long long *blk = nullptr;
  const size_t words = 2 + 1 + 1 + ((size_t)nedges + 1) + (size_t)nedges;
  char name_blk[32], name_pin[32];
  snprintf(name_blk, sizeof(name_blk), "bincount_blk%d", slot);
  snprintf(name_pin, sizeof(name_pin), "bincount_pin%d", slot);
  PRAD_TRY(c.get<unsigned long long>(name_blk, words, &blk));
  unsigned long long *keys = blk;
  int *info = (int *)(blk + 2), *top = (int *)(blk + 3);
  unsigned long long *cnt_d = blk + 4;
  double *e_d = (double *)(blk + 4 + (size_t)nedges + 1);
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned(name_pin, sizeof(unsigned long long) * (words + 2), &pin));
  unsigned long long *h = (unsigned long long *)pin;
  PRAD_HIP(hipMemsetAsync(blk, 0, sizeof(unsigned long long) * words, s));
  h[words] = ~0ull;
  h[words + 1] = 0ull;
  PRAD_HIP(hipMemcpyAsync(keys, h + words, 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  static const int cap = getenv("PRAD_MINMAX_BLOCKS") ? atoi(getenv("PRAD_MINMAX_BLOCKS")) : 512;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap));
  switch (dtype) {
    case 0: hipLaunchKernelGGL(roi_minmax_kernel<float>, dim3(gx), dim3(256), 0, s, (const float *)image, mask, n, keys); break;
    case 1: hipLaunchKernelGGL(roi_minmax_kernel<double>, dim3(gx), dim3(256), 0, s, (const double *)image, mask, n, keys); break;
    case 2: hipLaunchKernelGGL(roi_minmax_kernel<int>, dim3(gx), dim3(256), 0, s, (const int *)image, mask, n, keys); break;
    default: hipLaunchKernelGGL(roi_minmax_kernel<short>, dim3(gx), dim3(256), 0, s, (const short *)image, mask, n, keys); break;
  }
  if (dtype == 0)
    hipLaunchKernelGGL(bincount_edges_kernel<true>, dim3(1), dim3(256), 0, s, (const unsigned long long *)keys, binCount, e_d, info);
  else
    hipLaunchKernelGGL(bincount_edges_kernel<false>, dim3(1), dim3(256), 0, s, (const unsigned long long *)keys, binCount, e_d, info);
  PRAD_TRY(check_launch("bincount_edges_kernel"));
  switch (dtype) {
    case 0: PRAD_TRY(launch_digitize((const float *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    case 1: PRAD_TRY(launch_digitize((const double *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    case 2: PRAD_TRY(launch_digitize((const int *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
    default: PRAD_TRY(launch_digitize((const short *)image, mask, n, e_d, nedges, levels, top, cnt_d, s)); break;
  }
  PRAD_HIP(hipMemcpyAsync(h, blk, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, s));
  *host_out = h;
  return PRAD_OK;
}
int bincount_collect(const unsigned long long *h, int nedges, double *minmax, double *edges, int *max_level, long long *counts) {
  if (h[1] == 0ull) return fail(PRAD_E_ARG, "roi_minmax: empty ROI");
  minmax[0] = f64_unkey(h[0]);
  minmax[1] = f64_unkey(h[1]);
  if (*(const int *)(h + 2))
    return fail(PRAD_E_UNSUPPORTED, "bincount: constant or non-finite ROI (np.histogram widens the range: host-built edges)");
  if (max_level) *max_level = *(const int *)(h + 3);
  if (counts) memcpy(counts, h + 4, sizeof(long long) * ((size_t)nedges + 1));
  if (edges) memcpy(edges, h + 4 + (size_t)nedges + 1, sizeof(double) * nedges);
  return PRAD_OK;
}
}  // namespace

int prad_bincount_dev(const void *image, int dtype, const uint8_t *mask, long long n, int binCount, int32_t *levels,
                      double *minmax, double *edges, int *max_level, long long *counts, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!image || !mask || !levels || !minmax || n < 1) return fail(PRAD_E_ARG, "bincount: bad arguments");
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "bincount: dtype %d", dtype);
  if (binCount < 1 || binCount > 4096) return fail(PRAD_E_UNSUPPORTED, "bincount: binCount %d outside [1, 4096]", binCount);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *h = nullptr;
  PRAD_TRY(bincount_queue(c, PRAD_BIN_SLOTS, image, dtype, mask, n, binCount, levels, s, &h));   // (a block of its own: no ticket)
  PRAD_HIP(hipStreamSynchronize(s));
  return bincount_collect(h, binCount + 1, minmax, edges, max_level, counts);
}

// prad_bincount_dev in two halves (round 6: the case pipeline bins image i + 1 while the host still works on image i): the
// queueing half returns a ticket, prad_bincount_wait(ticket, ...) waits for THAT work only (an event behind its copy) and hands
// over what prad_bincount_dev returns.  Up to four tickets per thread; a ticket must be waited for exactly once.
int prad_bincount_enqueue_dev(const void *image, int dtype, const uint8_t *mask, long long n, int binCount, int32_t *levels,
                              int *ticket, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!image || !mask || !levels || !ticket || n < 1) return fail(PRAD_E_ARG, "bincount_enqueue: bad arguments");
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "bincount_enqueue: dtype %d", dtype);
  if (binCount < 1 || binCount > 4096) return fail(PRAD_E_UNSUPPORTED, "bincount_enqueue: binCount %d outside [1, 4096]", binCount);
  BinSlots &b = bin_slots();
  if (b.device != c.device) {
    for (int t = 0; t < PRAD_BIN_SLOTS; t++) {
      if (b.done[t]) (void)hipEventDestroy(b.done[t]);
      PRAD_HIP(hipEventCreateWithFlags(&b.done[t], hipEventDisableTiming));
      b.used[t] = false;
    }
    b.device = c.device;
  }
  const int t = (int)(b.seq % PRAD_BIN_SLOTS);
  if (b.used[t]) return fail(PRAD_E_ARG, "bincount_enqueue: %d binnings are in flight on this thread; prad_bincount_wait one first", PRAD_BIN_SLOTS);
  hipStream_t s = (hipStream_t)stream;
  PRAD_TRY(bincount_queue(c, t, image, dtype, mask, n, binCount, levels, s, &b.host[t]));
  PRAD_HIP(hipEventRecord(b.done[t], s));
  b.nedges[t] = binCount + 1;
  b.used[t] = true;
  b.seq++;
  *ticket = t;
  return PRAD_OK;
}

int prad_bincount_wait(int ticket, double *minmax, double *edges, int *max_level, long long *counts) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  BinSlots &b = bin_slots();
  if (ticket < 0 || ticket >= PRAD_BIN_SLOTS || !b.used[ticket] || !minmax) return fail(PRAD_E_ARG, "bincount_wait: ticket %d", ticket);
  b.used[ticket] = false;
  PRAD_HIP(hipEventSynchronize(b.done[ticket]));
  return bincount_collect(b.host[ticket], b.nedges[ticket], minmax, edges, max_level, counts);
}

int prad_digitize_dev(const void *image, int dtype, const uint8_t *mask, long long n, const double *edges, int nedges,
                      int32_t *levels, int *max_level, void *stream) {
  return prad_digitize_counts_dev(image, dtype, mask, n, edges, nedges, levels, max_level, nullptr, stream);
}

int prad_level_counts_dev(const int32_t *levels, const uint8_t *mask, long long n, int Ng, long long *counts,
                          void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!levels || !mask || !counts || n < 1 || Ng < 1) return fail(PRAD_E_ARG, "level_counts: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *d = nullptr;
  const size_t nb = (size_t)Ng + 1;
  PRAD_TRY(c.get<unsigned long long>("level_counts", nb, &d));
  PRAD_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long) * nb, s));
  // per-block partial sums are 32-bit: a block sees at most n / grid voxels, bounded below 2^32 by the grid size
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 1024));   // (flush atomics: see launch_digitize)
  const int use_lds = 4 * nb * sizeof(unsigned) <= 48 * 1024;
  hipLaunchKernelGGL(level_counts_kernel, dim3(gx), dim3(256), use_lds ? 4 * nb * sizeof(unsigned) : 0, s, levels, mask,
                     n, Ng, use_lds, d);
  PRAD_TRY(check_launch("level_counts_kernel"));
  PRAD_HIP(hipMemcpyAsync(counts, d, sizeof(long long) * nb, hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  return PRAD_OK;
}
}  // extern "C"
