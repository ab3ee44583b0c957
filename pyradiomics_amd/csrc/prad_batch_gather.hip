// prad_batch_gather.hip -- C ABI of the batched ROI gather (include/pyradiomics_amd.h: prad_batch_gather_dev); translation unit
// of libpyradiomics_amd.so.
#include <type_traits>

#include "kernels_batch_gather.h"

#include <algorithm>

using namespace prad;

namespace {

// bytes per element of the image dtype codes (0 float32, 1 float64, 2 int32, 3 int16) and of the label codes (2 int32,
// 3 int16, 4 uint8); 0 = not such a type
int image_bytes(int dtype) { return dtype == 0 || dtype == 2 ? 4 : (dtype == 1 ? 8 : (dtype == 3 ? 2 : 0)); }
int label_bytes(int dtype) { return dtype == 2 ? 4 : (dtype == 3 ? 2 : (dtype == 4 ? 1 : 0)); }

template <typename T, typename L>
int launch(hipStream_t s, unsigned blocks, const void *image, const void *labelmap, const GatherRoi *rois, const int *first,
           long long total, long long sy, long long sz, void *out_image, unsigned char *out_mask) {
  hipLaunchKernelGGL((batch_gather_kernel<T, L>), dim3(blocks), dim3(PRAD_GATHER_THREADS), 0, s, (const T *)image,
                     (const L *)labelmap, rois, first, total, sy, sz, (T *)out_image, out_mask);
  return check_launch("batch_gather_kernel");
}

template <typename T>
int launch_labels(int label_dtype, hipStream_t s, unsigned blocks, const void *image, const void *labelmap, const GatherRoi *rois,
                  const int *first, long long total, long long sy, long long sz, void *out_image, unsigned char *out_mask) {
  if (!labelmap) return launch<T, GatherNone>(s, blocks, image, nullptr, rois, first, total, sy, sz, out_image, nullptr);
  switch (label_dtype) {
    case 2: return launch<T, int>(s, blocks, image, labelmap, rois, first, total, sy, sz, out_image, out_mask);
    case 3: return launch<T, short>(s, blocks, image, labelmap, rois, first, total, sy, sz, out_image, out_mask);
    default: return launch<T, unsigned char>(s, blocks, image, labelmap, rois, first, total, sy, sz, out_image, out_mask);
  }
}

}  // namespace

extern "C" int prad_batch_gather_dev(const void *image, int image_dtype, const void *labelmap, int label_dtype, const int *size,
                                     int B, const int *labels, const int *lo, const int *box, const long long *offsets,
                                     void *out_image, unsigned char *out_mask, void *stream) {
  // ---- host checks: nothing is launched unless every box lies in the volume and the packed pieces follow one another ----
  if ((image == nullptr) != (out_image == nullptr) || (labelmap == nullptr) != (out_mask == nullptr))
    return fail(PRAD_E_ARG, "batch gather: an input without its output (or the reverse)");
  if (!image && !labelmap) return fail(PRAD_E_ARG, "batch gather: neither image nor label map");
  if (image && !image_bytes(image_dtype))
    return fail(PRAD_E_ARG, "batch gather: image dtype code %d (0 float32, 1 float64, 2 int32, 3 int16)", image_dtype);
  if (labelmap && !label_bytes(label_dtype))
    return fail(PRAD_E_ARG, "batch gather: label dtype code %d (2 int32, 3 int16, 4 uint8)", label_dtype);
  if (!size || !lo || !box || !offsets || (labelmap && !labels)) return fail(PRAD_E_ARG, "batch gather: NULL table");
  if (B < 1) return fail(PRAD_E_ARG, "batch gather: B=%d", B);
  for (int d = 0; d < 3; d++)
    if (size[d] < 1) return fail(PRAD_E_ARG, "batch gather: size[%d]=%d < 1", d, size[d]);
  const long long sy = size[2], sz = (long long)size[1] * size[2];
  std::vector<GatherRoi> rois((size_t)B);
  long long total = 0, end = 0;
  for (int b = 0; b < B; b++) {
    const int *l = lo + 3 * b, *x = box + 3 * b;
    for (int d = 0; d < 3; d++) {
      if (x[d] < 1) return fail(PRAD_E_ARG, "batch gather: ROI %d has extent[%d]=%d < 1", b, d, x[d]);
      if (l[d] < 0 || (long long)l[d] + x[d] > size[d])
        return fail(PRAD_E_ARG, "batch gather: ROI %d leaves the volume along axis %d (%d + %d > %d)", b, d, l[d], x[d], size[d]);
    }
    if (offsets[b] < end)
      return fail(PRAD_E_ARG, "batch gather: offsets[%d]=%lld lies before the end of ROI %d (%lld)", b, offsets[b], b - 1, end);
    GatherRoi &r = rois[(size_t)b];
    r.w = total;
    r.n = (long long)x[0] * x[1] * x[2];
    r.off = offsets[b];
    r.src = l[0] * sz + l[1] * sy + l[2];
    r.ny = x[1];
    r.nx = x[2];
    r.label = labels ? labels[b] : 0;      // (also without a label map: the masks' call and the images' calls share one table)
    r.pad = 0;
    total += r.n;
    end = r.off + r.n;
  }
  const long long nchunks = (total + PRAD_GATHER_CHUNK - 1) / PRAD_GATHER_CHUNK;
  if (nchunks > 2147483647LL) return fail(PRAD_E_UNSUPPORTED, "batch gather: %lld voxels in one call", total);
  // the ROI of every chunk's first item, and B - 1 behind the last chunk
  const size_t roi_bytes = sizeof(GatherRoi) * (size_t)B, first_bytes = sizeof(int) * (size_t)(nchunks + 1);
  std::vector<char> table(roi_bytes + first_bytes);
  {
    int *first = (int *)(table.data() + roi_bytes);      // (roi_bytes is a multiple of 16)
    int b = 0;
    for (long long c = 0; c < nchunks; c++) {
      const long long item = c * PRAD_GATHER_CHUNK;
      while (b + 1 < B && rois[(size_t)b + 1].w <= item) b++;
      first[c] = b;
    }
    first[nchunks] = B - 1;
    memcpy(table.data(), rois.data(), roi_bytes);
  }

  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  // The table stays on the device between calls: the masks and every derived image of one label map are gathered with the
  // same boxes, so only the first call of such a series uploads (a copy from pageable memory blocks the host while it is
  // staged; the buffer may be reused as soon as the call returns).
  char *prev = nullptr;
  {
    auto it = c.bufs.find(c.key("batch_gather_table"));
    if (it != c.bufs.end()) prev = (char *)it->second.p;
  }
  char *d_table = nullptr;
  PRAD_TRY(c.get<char>("batch_gather_table", table.size(), &d_table));
  TableCache &cached = c.tables_cached[c.key("batch_gather_table")];
  PRAD_TRY(c.begin_call(s));
  if (!(prev == d_table && cached.stream == (void *)s && cached.bytes == table)) {
    cached.bytes.clear();      // (a failing copy leaves nothing that could be taken for current)
    PRAD_HIP(hipMemcpyAsync(d_table, table.data(), table.size(), hipMemcpyHostToDevice, s));
    cached.bytes.swap(table);
    cached.stream = (void *)s;
  }
  const GatherRoi *d_rois = (const GatherRoi *)d_table;
  const int *d_first = (const int *)(d_table + roi_bytes);
  int rc;
  {
    Timed t(c, "batch_gather", s);
    const unsigned blocks = (unsigned)nchunks;
    if (!image) rc = launch_labels<GatherNone>(label_dtype, s, blocks, nullptr, labelmap, d_rois, d_first, total, sy, sz, nullptr, out_mask);
    else if (image_bytes(image_dtype) == 2) rc = launch_labels<unsigned short>(label_dtype, s, blocks, image, labelmap, d_rois, d_first, total, sy, sz, out_image, out_mask);
    else if (image_bytes(image_dtype) == 4) rc = launch_labels<unsigned>(label_dtype, s, blocks, image, labelmap, d_rois, d_first, total, sy, sz, out_image, out_mask);
    else rc = launch_labels<unsigned long long>(label_dtype, s, blocks, image, labelmap, d_rois, d_first, total, sy, sz, out_image, out_mask);
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  c.last_path = "batch";
  c.last_variant = "batch-gather";
  return PRAD_OK;
}
