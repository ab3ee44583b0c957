// prad_batch_common.h -- the host layer the batched small-ROI translation units (prad_batch*.hip) share: the checks of the
// `sizes` / `off` arguments, the per-ROI record table with its one upload, the call sequence around the launches and the
// dispatch over the image dtype codes.  Host only: no kernel lives here, and nothing here is a symbol the library exports.
#pragma once

#include "prad_runtime.h"

namespace prad {

static inline long long roi_nvox(const int *sizes, int b) { return (long long)sizes[3 * b] * sizes[3 * b + 1] * sizes[3 * b + 2]; }

// B and the `sizes` pointer; min_B: 0 where an empty batch is a valid call, 1 where it is not.  `what` is the message prefix.
static inline int roi_count_check(const char *what, const int *sizes, int B, int min_B) {
  if (B < min_B || (B > 0 && !sizes)) return fail(PRAD_E_ARG, "%s: B=%d, sizes=%p", what, B, (const void *)sizes);
  return PRAD_OK;
}

// every extent of every ROI is >= 1; *max_vox (may be NULL) = voxels of the largest box, at least 1
static inline int roi_sizes_check(const char *what, const int *sizes, int B, long long *max_vox) {
  long long most = 1;
  for (int b = 0; b < B; b++) {
    for (int d = 0; d < 3; d++)
      if (sizes[3 * b + d] < 1) return fail(PRAD_E_ARG, "%s: ROI %d has size[%d]=%d < 1", what, b, d, sizes[3 * b + d]);
    const long long n = roi_nvox(sizes, b);
    most = n > most ? n : most;
  }
  if (max_vox) *max_vox = most;
  return PRAD_OK;
}

static inline int roi_offsets_check(const char *what, const long long *off, int B) {
  for (int b = 0; b < B; b++)
    if (off[b] < 0) return fail(PRAD_E_ARG, "%s: off[%d]=%lld < 0", what, b, off[b]);
  return PRAD_OK;
}

// The grey-level count of every ROI of a call: the host vector [B] of the *_ng entry points, or -- v == NULL -- one count for
// all of them (the scalar entry points, which so share the implementation without building a vector).
struct RoiLevels {
  const int *v;
  int all;
  int operator[](int b) const { return v ? v[b] : all; }
  int most(int B) const {
    if (!v) return all;
    int m = 1;
    for (int b = 0; b < B; b++) m = v[b] > m ? v[b] : m;
    return m;
  }
};

// every count is >= 1
static inline int roi_levels_check(const char *what, const RoiLevels &Ng, int B) {
  if (!Ng.v) return Ng.all < 1 ? fail(PRAD_E_ARG, "%s: Ng=%d < 1", what, Ng.all) : (int)PRAD_OK;
  for (int b = 0; b < B; b++)
    if (Ng.v[b] < 1) return fail(PRAD_E_ARG, "%s: ROI %d has Ng=%d < 1", what, b, Ng.v[b]);
  return PRAD_OK;
}

// true when a count lies above `cap`; `why` (of `n` bytes) then says which
static inline bool roi_levels_above(const RoiLevels &Ng, int B, int cap, char *why, size_t n) {
  if (!Ng.v) {
    if (Ng.all > cap) snprintf(why, n, "Ng=%d above %d", Ng.all, cap);
    return Ng.all > cap;
  }
  for (int b = 0; b < B; b++)
    if (Ng.v[b] > cap) {
      snprintf(why, n, "ROI %d has Ng=%d above %d", b, Ng.v[b], cap);
      return true;
    }
  return false;
}

// The per-ROI records of one call: a pinned host block the entry point fills and the device block the kernel reads, both kept
// under the workspace name `slot`; `tail` more bytes (16-byte aligned) follow the records in the same upload.
template <typename Rec>
struct __attribute__((visibility("hidden"))) RecordTable {
  Rec *host = nullptr;
  const Rec *dev = nullptr;
  size_t bytes = 0, tail_at = 0;

  int reserve(Context &c, const char *slot, size_t count, size_t tail = 0) {
    tail_at = tail ? (sizeof(Rec) * count + 15) & ~(size_t)15 : sizeof(Rec) * count;
    bytes = tail_at + tail;
    void *h = nullptr, *d = nullptr;
    PRAD_TRY(c.get_pinned(slot, bytes, &h));
    PRAD_TRY(c.get(slot, bytes, &d));
    host = (Rec *)h;
    dev = (const Rec *)d;
    return PRAD_OK;
  }
  void *host_tail() const { return (char *)host + tail_at; }
  const void *dev_tail() const { return (const char *)dev + tail_at; }
  int upload(hipStream_t s) const {
    PRAD_HIP(hipMemcpyAsync((void *)dev, host, bytes, hipMemcpyHostToDevice, s));
    return PRAD_OK;
  }
};

// lets `kernel` ask for `lds` bytes of dynamic LDS where that is more than the 64 KiB every kernel may have
template <typename Kernel>
static int allow_dynamic_lds(Kernel *kernel, size_t lds) {
  if (lds > 64 * 1024)
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return PRAD_OK;
}

// One batched call on stream s: the table's upload, then `launches` -- a callable that brackets its kernels with a Timed of its
// own and returns their status -- between begin_call and end_call; the call is closed whether or not they succeed.  The host then
// waits for the stream (the pinned record block is reused by the next call) and the route is recorded.
template <typename Rec, typename Launches>
static int batch_call(Context &c, hipStream_t s, const RecordTable<Rec> &table, const char *variant, Launches &&launches) {
  PRAD_TRY(c.begin_call(s));
  int rc = table.upload(s);
  if (rc == PRAD_OK) rc = launches();
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));
  c.last_path = "batch";
  c.last_variant = variant;
  return PRAD_OK;
}

// f(T()) for the element type T of an image dtype code: 0 float32, 1 float64, 2 int32, anything else int16 (callers have
// checked the code)
template <typename F>
static int dispatch_image_dtype(int dtype, F &&f) {
  switch (dtype) {
    case 0: return f(float());
    case 1: return f(double());
    case 2: return f(int());
    default: return f(short());
  }
}

}  // namespace prad
