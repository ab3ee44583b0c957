// prad_labels.hip -- C ABI of the label census (include/pyradiomics_amd.h: prad_label_census*, prad_mask_max_dev);
// translation unit of libpyradiomics_amd.so.
#include "kernels_labels.h"

#include <algorithm>

using namespace prad;

namespace {

// compute units of the device this thread currently uses (asked per call: a thread may change devices between calls)
int cu_count() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}

// bytes per element of the integer dtype codes (include/pyradiomics_amd.h); 0 = not a label type
size_t label_bytes(int dtype) { return dtype == 2 ? 4 : (dtype == 3 ? 2 : (dtype == 4 ? 1 : 0)); }

template <typename T>
int launch_census(hipStream_t s, const T *mask, CensusGeo g, long long *table, bool lds) {
  // 4 voxels per lane (4 / 8 / 16-byte loads) when every lane's piece is aligned and inside one row
  const bool vec = g.nx % 4 == 0 && ((uintptr_t)mask % (4 * sizeof(T))) == 0;
  const int V = vec ? 4 : 1;
  g.nchunks = (g.nx + 64 * V - 1) / (64 * V);
  g.items = (long long)g.nz * g.ny * g.nchunks;
  const int waves = PRAD_CENSUS_THREADS / 64;
  const size_t lds_bytes = lds ? sizeof(int) * (size_t)(g.max_label + 1) * (1 + 2 * g.nd) : 0;
  // enough workgroups to fill the CUs (4 per CU, 2 when each has a large table to clear and merge), but no wave with
  // less than one round of loads
  const long long want = (g.items + (long long)waves * PRAD_CENSUS_INFLIGHT - 1) / ((long long)waves * PRAD_CENSUS_INFLIGHT);
  const long long cap = (long long)cu_count() * (lds_bytes > 16384 ? 2 : 4);
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min(want, cap));
  g.per_wave = (g.items + (long long)blocks * waves - 1) / ((long long)blocks * waves);
  const unsigned ib = (unsigned)std::min<long long>(256, ((long long)(g.max_label + 1) * (1 + 2 * g.nd) + 255) / 256);
  hipLaunchKernelGGL(census_init_kernel, dim3(ib), dim3(256), 0, s, table, g);
  PRAD_TRY(check_launch("census_init_kernel"));
#define PRAD_CENSUS(VV, LL) \
  hipLaunchKernelGGL((label_census_kernel<T, VV, LL>), dim3(blocks), dim3(PRAD_CENSUS_THREADS), lds_bytes, s, mask, g, table)
  if (vec && lds) PRAD_CENSUS(4, true);
  else if (vec) PRAD_CENSUS(4, false);
  else if (lds) PRAD_CENSUS(1, true);
  else PRAD_CENSUS(1, false);
#undef PRAD_CENSUS
  return check_launch("label_census_kernel");
}

template <typename T>
int launch_max(hipStream_t s, const T *p, long long n, long long *out) {
  hipLaunchKernelGGL(set_ll_kernel, dim3(1), dim3(1), 0, s, out, -9223372036854775807LL - 1);
  PRAD_TRY(check_launch("set_ll_kernel"));
  const long long vecs = n / (16 / (long long)sizeof(T)) + 1;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((vecs + 255) / 256, (long long)cu_count() * 8));
  hipLaunchKernelGGL(mask_max_kernel<T>, dim3(blocks), dim3(256), 0, s, p, n, out);
  return check_launch("mask_max_kernel");
}

}  // namespace

extern "C" int prad_label_census_dev(const void *mask, int dtype, const int *size, int Nd, int max_label, long long *table,
                                     void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!mask || !size || !table) return fail(PRAD_E_ARG, "label census: NULL pointer");
  if (Nd != 2 && Nd != 3) return fail(PRAD_E_ARG, "label census: Nd=%d (2 or 3)", Nd);
  if (!label_bytes(dtype)) return fail(PRAD_E_ARG, "label census: dtype code %d (2 int32, 3 int16, 4 uint8)", dtype);
  if (max_label < 0 || max_label > PRAD_CENSUS_MAX_LABEL)
    return fail(PRAD_E_ARG, "label census: max_label=%d outside [0, %d]", max_label, PRAD_CENSUS_MAX_LABEL);
  Geo geo;
  PRAD_TRY(make_geo(size, Nd, &geo));
  CensusGeo g;
  g.nd = Nd;
  g.nz = Nd == 3 ? size[0] : 1;
  g.ny = size[Nd - 2];
  g.nx = size[Nd - 1];
  g.max_label = max_label;
  g.nchunks = 0;
  g.items = g.per_wave = 0;
  const bool lds = (long long)(max_label + 1) * (1 + 2 * Nd) <= PRAD_CENSUS_LDS_WORDS;
  hipStream_t s = (hipStream_t)stream;
  PRAD_TRY(c.begin_call(s));
  int rc;
  {
    Timed t(c, "label_census", s);
    rc = dtype == 2 ? launch_census<int>(s, (const int *)mask, g, table, lds)
         : dtype == 3 ? launch_census<short>(s, (const short *)mask, g, table, lds)
                      : launch_census<unsigned char>(s, (const unsigned char *)mask, g, table, lds);
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));
  c.last_path = "label_census";
  c.last_variant = lds ? "census-lds" : "census-global";
  return PRAD_OK;
}

extern "C" int prad_label_census(const void *mask, int dtype, const int *size, int Nd, int max_label, long long *table) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!mask || !size || !table) return fail(PRAD_E_ARG, "label census: NULL pointer");
  if (!label_bytes(dtype)) return fail(PRAD_E_ARG, "label census: dtype code %d (2 int32, 3 int16, 4 uint8)", dtype);
  if (max_label < 0 || max_label > PRAD_CENSUS_MAX_LABEL)
    return fail(PRAD_E_ARG, "label census: max_label=%d outside [0, %d]", max_label, PRAD_CENSUS_MAX_LABEL);
  if (Nd != 2 && Nd != 3) return fail(PRAD_E_ARG, "label census: Nd=%d (2 or 3)", Nd);
  Geo geo;
  PRAD_TRY(make_geo(size, Nd, &geo));
  const size_t bytes = (size_t)geo.n * label_bytes(dtype), words = (size_t)(max_label + 1) * (1 + 2 * Nd);
  void *d_mask = nullptr;
  long long *d_table = nullptr;
  PRAD_TRY(c.get("labels_mask", bytes, &d_mask));
  PRAD_TRY(c.get<long long>("labels_table", words, &d_table));
  PRAD_HIP(hipMemcpyAsync(d_mask, mask, bytes, hipMemcpyHostToDevice, c.own_stream));
  PRAD_TRY(prad_label_census_dev(d_mask, dtype, size, Nd, max_label, d_table, c.own_stream));
  PRAD_HIP(hipMemcpyAsync(table, d_table, sizeof(long long) * words, hipMemcpyDeviceToHost, c.own_stream));
  PRAD_HIP(hipStreamSynchronize(c.own_stream));
  return PRAD_OK;
}

extern "C" int prad_mask_max_dev(const void *mask, int dtype, long long n, long long *max_value, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!mask || !max_value || n < 1) return fail(PRAD_E_ARG, "mask max: NULL pointer or empty array");
  if (!label_bytes(dtype)) return fail(PRAD_E_ARG, "mask max: dtype code %d (2 int32, 3 int16, 4 uint8)", dtype);
  hipStream_t s = (hipStream_t)stream;
  long long *d_out = nullptr;
  PRAD_TRY(c.get<long long>("labels_max", 1, &d_out));
  PRAD_TRY(c.begin_call(s));
  int rc;
  {
    Timed t(c, "mask_max", s);
    rc = dtype == 2 ? launch_max<int>(s, (const int *)mask, n, d_out)
         : dtype == 3 ? launch_max<short>(s, (const short *)mask, n, d_out)
                      : launch_max<unsigned char>(s, (const unsigned char *)mask, n, d_out);
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipMemcpyAsync(max_value, d_out, sizeof(long long), hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  return PRAD_OK;
}
