// prad_glszm.hip -- grey-level size-zone matrix (cmatrices.c:94-297): the kernels, their drivers and the entry points that take
// device arrays (the two host-array wrappers stay with the staging code in prad_api.hip).
// Segment mode (one box = the whole array): zones are the connected components of equal-level masked voxels under the angle
// set.  prad_glszm_plan.h chooses the route from the call's shape: the DENSE model (kernels_glszm_dense.h) serves the full 26- or
// in-plane 8-neighbourhood with levels that fit a byte, a LABEL VOLUME (kernels_glszm_labels.h) everything else.  Voxel mode
// (many small boxes): kernels_glszm_voxel.h.  Phase 1 leaves the zones on the device (ZoneState); the follow-up calls -- fill,
// distinct sizes, compact fill, ordered zone list -- read them through the struct of the model that is live.
#include "prad_runtime.h"
#include "prad_glszm_plan.h"
#include "kernels_glszm_labels.h"
#include "kernels_glszm_dense.h"
#include "kernels_glszm_zones.h"
#include "kernels_glszm_voxel.h"
#include "prad_internal.h"

#include <algorithm>
#include <cmath>

using namespace prad;

namespace {

// ---- zone state: phase 1 -> the follow-up calls --------------------------------------------------------------------------
enum ZoneModel { ZONES_NONE, ZONES_DENSE, ZONES_LABELS, ZONES_VOXEL };
struct DenseZones {
  int *vid = nullptr;              // [n] voxel -> dense id of its tile root; once `published`: the zone list's label-volume view
  unsigned *tsize = nullptr;       // [idcap] zone size at the zone root's id
  int *parent = nullptr;           // [idcap] dense union-find, nearly flat after glszm_rootsum_dense_kernel
  unsigned *tinfo = nullptr;       // [idcap] dense id -> voxels of the tile component | grey level << 16
  int *rootctl = nullptr;          // [0] tile roots, [2] pairs in the work list, [3] work list overflow
  size_t idcap = 0;                // entries the dense arrays hold (ids come in chunks: holes)
  bool published = false;          // the ordered zone list has turned vid[] into its label-volume view
};
struct LabelZones { int *labels = nullptr; unsigned *sizes = nullptr; };     // [n] root label or -1, [n] zone size at the root's index
struct VoxelZones {
  int *zones = nullptr;            // [boxmax][2][nvox] (level, size) interleaved by kernel
  int *zone_count = nullptr;       // [nvox]
  long long boxmax = 0;
};
struct ZoneState {
  ZoneModel model = ZONES_NONE;    // which of dense / vol / vox is live: the only one read
  bool valid = false;              // the synchronous phase 1 has completed: the host-side follow-ups may run
  GlszmRoute route = GLSZM_LABEL_VOLUME;
  int device = -1, nvox = 0, max_region = 0;
  long long nzones = 0;
  Geo g;
  DenseZones dense; LabelZones vol; VoxelZones vox;
  // segment mode, either model
  const int32_t *image = nullptr;  // levels are read from the image at fill time
  int nsizes = -1;                 // distinct zone sizes found by prad_glszm_sizes (-1 = not run)
  int nsmall = 0, nlarge = 0;      //   ... of which below / at or above PRAD_SMALL_SIZES
  unsigned *small_bits = nullptr;  // bitmap of the zone sizes < PRAD_SMALL_SIZES that occur
  int *large_list = nullptr, *large_count = nullptr;     // every zone size >= PRAD_SMALL_SIZES (unsorted, with repeats)
  int large_cap = 0;
  int *small_rank = nullptr;       // after prad_glszm_sizes / glszm_rank_kernel: size -> compact column
  bool segment() const { return model == ZONES_DENSE || model == ZONES_LABELS; }
};
ZoneState &zone_state() {
  static thread_local ZoneState s;
  return s;
}

// What the kernels of kernels_glszm_zones.h are handed for the live segment model: a label volume passes null for the three
// dense arrays.  The one place that decides it.
struct ZoneArgs {
  int *labels;
  const unsigned *sizes, *tinfo;
  const int *parent, *rootctl;
};
ZoneArgs zone_args(const ZoneState &st) {
  if (st.model == ZONES_DENSE) return {st.dense.vid, st.dense.tsize, st.dense.tinfo, st.dense.parent, st.dense.rootctl};
  return {st.vol.labels, st.vol.sizes, nullptr, nullptr, nullptr};
}

unsigned glszm_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192)); }

// ---- phase 1, segment mode ------------------------------------------------------------------------------------------------
// one segment-mode call: its arguments and the workspace every route uses
struct SegmentCall {
  Context &c; hipStream_t s; const Geo &g;
  const int32_t *image; const uint8_t *mask;
  int Na, Ng;
  int *angles_d = nullptr;
  int *labels = nullptr;           // "glszm_labels": the label volume, or vid[] of the dense model
  unsigned *sizes = nullptr;       // "glszm_sizes": sizes by voxel, or tsize[] of the dense model
  int *stats = nullptr, *stats_h = nullptr;        // [0] largest zone, [1] voxel mode: scratch overflow, [2..3] zone count (64 bit)
  int *flags_d = nullptr, *flags_h = nullptr;      // dense routes: [0] != 0, a masked level outside 1..Ng (found by the pack)
};

int stats_begin(Context &c, hipStream_t s, int **stats, int **stats_h) {
  PRAD_TRY(c.get<int>("glszm_stats", 8, stats));
  PRAD_HIP(hipMemsetAsync(*stats, 0, sizeof(int) * 8, s));
  return c.get_pinned("glszm_stats_h", sizeof(int) * 8, (void **)stats_h);
}

int segment_begin(SegmentCall &k, const int *angles_h, ZoneState &st) {
  Context &c = k.c;
  const Geo &g = k.g;
  st.valid = false; st.model = ZONES_NONE;
  PRAD_TRY(stats_begin(c, k.s, &k.stats, &k.stats_h));
  PRAD_TRY(c.get<int>("angles", (size_t)k.Na * g.nd, &k.angles_d));
  PRAD_HIP(hipMemcpyAsync(k.angles_d, angles_h, sizeof(int) * k.Na * g.nd, hipMemcpyHostToDevice, k.s));
  PRAD_TRY(c.get<int>("glszm_labels", (size_t)g.n, &k.labels));
  PRAD_TRY(c.get<unsigned>("glszm_sizes", (size_t)g.n, &k.sizes));
  st.large_cap = (int)(g.n / PRAD_SMALL_SIZES + 2);
  PRAD_TRY(c.get<unsigned>("glszm_small_bits", PRAD_SMALL_SIZES / 32, &st.small_bits));
  PRAD_TRY(c.get<int>("glszm_large_list", (size_t)st.large_cap, &st.large_list));
  PRAD_TRY(c.get<int>("glszm_large_count", 1, &st.large_count));
  return ZeroBatch().add(st.small_bits, PRAD_SMALL_SIZES / 8).add(st.large_count, sizeof(int)).launch(k.s);
}

// the flag words of a dense call: a masked level outside 1..Ng (flags[0], found by the pack) sends it through the int32 kernels
int segment_flags(SegmentCall &k) {
  PRAD_TRY(k.c.get<int>("flags", 4, &k.flags_d));
  return k.c.get_pinned("glszm_flags_h", sizeof(int) * 4, (void **)&k.flags_h);
}

// The dense model: glszm_tile8_kernel lists the cross-tile pairs (it holds the levels with their halo in LDS),
// glszm_pairs_kernel unites the tile roots; a full work list (decided on the device: rootctl[3]) sends the call through
// glszm_border8d_kernel instead.  PRAD_GLSZM_WORKCAP: a test hook -- a tiny list forces that route.
template <int MODE>
int zones_dense(SegmentCall &k, const GlszmPlan &p, ZoneState &st) {
  Context &c = k.c;
  const Geo &g = k.g;
  hipStream_t s = k.s;
  DenseZones &d = st.dense = DenseZones();
  st.model = ZONES_DENSE;
  d.vid = k.labels;
  d.tsize = k.sizes;
  d.idcap = (size_t)g.n;
  uint8_t *levels = nullptr;
  const char *wcap = getenv("PRAD_GLSZM_WORKCAP");
  const int workcap = wcap ? std::max(1, atoi(wcap)) : (int)std::min<long long>(1LL << 30, std::max<long long>(g.n, 65536));
  int2 *work = nullptr;
  // lanes of glszm_pairs_kernel: MORE of them are slower on structured volumes (they collide in the trees of the
  // large zones: 256^3 smooth 273 us with 2048 workgroups, 121 with 384; 512^3 790 / 612 with 768)
  static const int pgrid_env = getenv("PRAD_GLSZM_PGRID") ? atoi(getenv("PRAD_GLSZM_PGRID")) : 0;
  const int pgrid = pgrid_env > 0 ? pgrid_env : (int)std::min(2048.0, std::max(64.0, 1.5 * std::cbrt((double)g.n)));
  PRAD_TRY(c.get<int>("glszm_parent", (size_t)g.n, &d.parent));
  PRAD_TRY(c.get<unsigned>("glszm_tinfo", (size_t)g.n, &d.tinfo));
  PRAD_TRY(c.get<int>("glszm_rootctl", 4, &d.rootctl));
  PRAD_TRY(c.get<int2>("glszm_worklist", (size_t)workcap, &work));
  PRAD_TRY(ZeroBatch().add(k.flags_d, sizeof(int) * 4).add(d.rootctl, sizeof(int) * 4).launch(s));
  PRAD_TRY(glszm_byte_pack(c, s, g, k.image, k.mask, k.Ng, k.flags_d, &levels));
  const int *flags = k.flags_d, *rootctl = d.rootctl;
  const dim3 bgrid((unsigned)std::min<long long>(((long long)p.dims[0] * p.dims[1] + 3) / 4, 16384));
  hipLaunchKernelGGL(glszm_tile8_kernel<MODE>, dim3((unsigned)p.tiles), dim3(256), 0, s, levels, p.dims[0], p.dims[1], p.dims[2],
                     d.vid, flags, d.rootctl, d.tinfo, work, workcap);
  hipLaunchKernelGGL(glszm_dense_init_kernel, dim3(2048), dim3(256), 0, s, rootctl, (const unsigned *)d.tinfo, d.parent, d.tsize,
                     flags);
  hipLaunchKernelGGL(glszm_pairs_kernel, dim3(pgrid), dim3(256), 0, s, (const int2 *)work, rootctl, (const int *)d.vid, d.parent,
                     flags);
  hipLaunchKernelGGL(glszm_border8d_kernel<MODE>, bgrid, dim3(256), 0, s, levels, p.dims[0], p.dims[1], p.dims[2],
                     (const int *)d.vid, d.parent, flags, rootctl);
  hipLaunchKernelGGL(glszm_rootsum_dense_kernel, dim3(2048), dim3(256), 0, s, rootctl, d.parent, d.tsize, flags);
  return check_launch("glszm_tile8/pairs/rootsum_kernel");
}

// int32 tiles: zones labelled inside the tiles, united across their faces by the border kernel of the mode
int zones_tiles(SegmentCall &k, const GlszmPlan &p) {
  hipStream_t s = k.s;
  const int Nz = p.dims[0], Ny = p.dims[1], Nx = p.dims[2];
  const dim3 bgrid((unsigned)std::min<long long>(((long long)Nz * Ny + 3) / 4, 16384));
  hipLaunchKernelGGL(glszm_tile_kernel, dim3((unsigned)p.tiles), dim3(256), 0, s, p.A, p.mode, k.image, k.mask, Nz, Ny, Nx, k.labels,
                     k.sizes);
  PRAD_TRY(check_launch("glszm_tile_kernel"));
  if (p.route == GLSZM_TILES_FULL26)
    hipLaunchKernelGGL(glszm_border_full_kernel<1>, bgrid, dim3(256), 0, s, k.image, k.mask, Nz, Ny, Nx, k.labels);
  else if (p.route == GLSZM_TILES_FULL8)
    hipLaunchKernelGGL(glszm_border_full_kernel<2>, bgrid, dim3(256), 0, s, k.image, k.mask, Nz, Ny, Nx, k.labels);
  else
    hipLaunchKernelGGL(glszm_border_kernel, bgrid, dim3(256), 0, s, p.A, k.image, k.mask, Nz, Ny, Nx, k.labels);
  PRAD_TRY(check_launch("glszm_border_kernel"));
  hipLaunchKernelGGL(glszm_rootsum_kernel, dim3((unsigned)((k.g.n + PRAD_RS_CHUNK - 1) / PRAD_RS_CHUNK)), dim3(256), 0, s, k.g.n,
                     k.labels, k.sizes);
  return check_launch("glszm_rootsum_kernel");
}

// the label volume of any Nd and any angle set: one union per masked voxel and backward angle
int zones_label_volume(SegmentCall &k) {
  hipStream_t s = k.s;
  const long long n = k.g.n;
  hipLaunchKernelGGL(glszm_init_kernel, dim3(glszm_grid(n)), dim3(256), 0, s, k.mask, n, k.labels, k.sizes);
  PRAD_TRY(check_launch("glszm_init_kernel"));
  hipLaunchKernelGGL(glszm_merge_kernel, dim3(glszm_grid(n)), dim3(256), 0, s, k.g, k.angles_d, k.Na, k.image, k.mask, k.labels);
  PRAD_TRY(check_launch("glszm_merge_kernel"));
  hipLaunchKernelGGL(glszm_flatten_count_kernel, dim3(glszm_grid(n)), dim3(256), 0, s, n, k.labels, k.sizes);
  return check_launch("glszm_flatten_count_kernel");
}

// the launches of one route, then the zone statistics of its model
int segment_launch(SegmentCall &k, const GlszmPlan &p, ZoneState &st) {
  if (p.dense()) {
    PRAD_TRY(p.route == GLSZM_DENSE26 ? zones_dense<1>(k, p, st) : zones_dense<2>(k, p, st));
  } else {
    st.model = ZONES_LABELS;
    st.vol.labels = k.labels;
    st.vol.sizes = k.sizes;
    PRAD_TRY(p.tiled() ? zones_tiles(k, p) : zones_label_volume(k));
  }
  st.route = p.route;
  k.c.last_variant = glszm_route_name(p.route);
  const ZoneArgs z = zone_args(st);
  hipLaunchKernelGGL(glszm_stats_kernel, dim3(std::min(glszm_grid(k.g.n), 1024u)), dim3(256), 0, k.s, k.g.n, (const int *)z.labels,
                     z.sizes, k.stats, (unsigned long long *)(k.stats + 2), st.small_bits, st.large_list, st.large_cap,
                     st.large_count, (const int *)(p.dense() ? k.flags_d : nullptr), z.parent, z.rootctl);
  PRAD_TRY(check_launch("glszm_stats_kernel"));
  st.image = k.image; st.g = k.g;
  st.nvox = 1; st.device = k.c.device;
  return PRAD_OK;
}

// Segment-mode zones ENQUEUED only (prad_glszm_features_dev): a dense route or nothing (PRAD_E_UNSUPPORTED); no copy back, no
// synchronisation -- zone count, largest zone and the flags stay on the device ("glszm_stats", "flags").  The state stays
// invalid for the host-side follow-ups, which need the synchronous call.
int glszm_zones_enqueue(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, const int *angles_h,
                        int Na, int Ng) {
  ZoneState &st = zone_state();
  SegmentCall k{c, s, g, image, mask, Na, Ng};
  PRAD_TRY(segment_begin(k, angles_h, st));
  Timed t(c, "glszm", s);
  const GlszmPlan p = glszm_plan(g.size, g.nd, angles_h, Na, Ng);
  if (!p.dense()) return fail(PRAD_E_UNSUPPORTED, "GLSZM: the enqueue-only route needs the packed-byte tile kernels");
  PRAD_TRY(segment_flags(k));
  return segment_launch(k, p, st);
}

// ---- phase 1, voxel mode ---------------------------------------------------------------------------------------------------
int zones_voxel(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, const int *angles_h, int Na,
                int Ns, int Nvox, const int *voxels_dev, int kernelRadius, int force2Ddim, int *stats, ZoneState &st) {
  if (kernelRadius <= 0) return fail(PRAD_E_ARG, "Expecting kernelRadius > 0");
  long long b = 1;
  for (int d = 0; d < g.nd; d++)
    if (d != force2Ddim) b *= std::min<long long>(2LL * kernelRadius + 1, g.size[d]);
  const VoxMode vm{Nvox, voxels_dev, kernelRadius, force2Ddim, b};
  int *angles_d = nullptr;
  PRAD_TRY(c.get<int>("angles", (size_t)Na * g.nd, &angles_d));
  PRAD_HIP(hipMemcpyAsync(angles_d, angles_h, sizeof(int) * Na * g.nd, hipMemcpyHostToDevice, s));
  // _cmatrices.c:298-314: Ns is clipped to the nominal kernel volume (2r+1)^(Nd or Nd-1)
  long long nominal = 1;
  for (int d = 0; d < (force2Ddim >= 0 ? g.nd - 1 : g.nd); d++) nominal *= (2LL * kernelRadius + 1);
  const int Ns_eff = (int)std::min<long long>(Ns, nominal);
  uint8_t *visited = nullptr;
  int *stack = nullptr;
  VoxelZones &v = st.vox;
  PRAD_TRY(c.get<uint8_t>("glszm_visited", (size_t)b * Nvox, &visited));
  PRAD_TRY(c.get<int>("glszm_stack", (size_t)b * Nvox, &stack));
  PRAD_TRY(c.get<int>("glszm_zones", (size_t)b * 2 * Nvox, &v.zones));
  PRAD_TRY(c.get<int>("glszm_zone_count", (size_t)Nvox, &v.zone_count));
  Timed t(c, "glszm", s);
  hipLaunchKernelGGL(glszm_voxel_kernel, dim3((unsigned)((Nvox + 63) / 64)), dim3(64), 0, s, g, vm, image, mask, angles_d, Na,
                     visited, stack, v.zones, v.zone_count, stats, (unsigned long long *)(stats + 2), Ns_eff);
  PRAD_TRY(check_launch("glszm_voxel_kernel"));
  v.boxmax = b;
  st.model = ZONES_VOXEL; st.route = GLSZM_VOXEL;
  c.last_variant = glszm_route_name(GLSZM_VOXEL);
  st.g = g; st.nvox = Nvox; st.device = c.device;
  return PRAD_OK;
}

// ---- phase 1, synchronous: the zones of either mode; returns the largest zone (negative: an error) ------------------------
int glszm_zones(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, const int *angles_h, int Na,
                int Ng, int Ns, int Nvox, const int *voxels_dev, int kernelRadius, int force2Ddim, long long *nzones_out) {
  ZoneState &st = zone_state();
  int *stats = nullptr, *stats_h = nullptr;
  bool stats_copied = false;
  if (!voxels_dev) {
    if (Nvox != 1) return fail(PRAD_E_ARG, "Nvox=%d without a voxel list", Nvox);
    SegmentCall k{c, s, g, image, mask, Na, Ng};
    PRAD_TRY(segment_begin(k, angles_h, st));
    stats = k.stats, stats_h = k.stats_h;
    Timed t(c, "glszm", s);
    const GlszmPlan p = glszm_plan(g.size, g.nd, angles_h, Na, Ng);
    if (p.dense()) PRAD_TRY(segment_flags(k));
    PRAD_TRY(segment_launch(k, p, st));
    if (p.dense()) {
      PRAD_HIP(hipMemcpyAsync(k.flags_h, k.flags_d, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
      PRAD_HIP(hipMemcpyAsync(stats_h, stats, sizeof(int) * 8, hipMemcpyDeviceToHost, s));
      PRAD_HIP(hipStreamSynchronize(s));
      stats_copied = !k.flags_h[0];
      // irregular levels: nothing was computed, run the int32 kernels
      if (!stats_copied) PRAD_TRY(segment_launch(k, glszm_plan_int32(p), st));
    }
  } else {
    st.valid = false; st.model = ZONES_NONE;
    PRAD_TRY(stats_begin(c, s, &stats, &stats_h));
    PRAD_TRY(zones_voxel(c, s, g, image, mask, angles_h, Na, Ns, Nvox, voxels_dev, kernelRadius, force2Ddim, stats, st));
  }
  if (!stats_copied) {
    PRAD_HIP(hipMemcpyAsync(stats_h, stats, sizeof(int) * 8, hipMemcpyDeviceToHost, s));
    PRAD_HIP(hipStreamSynchronize(s));
  }
  st.max_region = stats_h[0];
  st.nsizes = -1;
  st.nzones = (long long)*(unsigned long long *)(stats_h + 2);
  st.valid = true;
  if (nzones_out) *nzones_out = st.nzones;
  // scratch-exhaustion rule of the reference (see include/pyradiomics_amd.h)
  if (st.segment() ? st.nzones >= 2LL * Ns : stats_h[1] != 0)
    return fail(PRAD_E_INDEX, "GLSZM: zone list would overflow the reference's Ns-sized scratch (Ns=%d)", Ns);
  c.last_path = st.segment() ? "glszm-unionfind" : "glszm-voxel";
  return st.max_region;
}

// ---- the follow-up calls ----------------------------------------------------------------------------------------------------
// the zones of the last synchronous phase 1 on this device, or null with the error recorded
ZoneState *live_state(Context &c, const char *what) {
  ZoneState &st = zone_state();
  if (!st.valid || st.model == ZONES_NONE || st.device != c.device) {
    fail(PRAD_E_ARG, "%s without a preceding prad_calculate_glszm", what);
    return nullptr;
  }
  c.last_variant = glszm_route_name(st.route);
  return &st;
}

// the error word of a fill kernel, read back: the reference's "index out of range"
int fill_verdict(Context &c, hipStream_t s, const int *err) {
  void *hp = nullptr;
  PRAD_TRY(c.get_pinned("glszm_err_h", sizeof(int) * 4, &hp));
  PRAD_HIP(hipMemcpyAsync(hp, err, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  return ((int *)hp)[0] ? PRAD_INDEX_ERROR : PRAD_OK;
}

// The compact fill, [Ng][k] over the distinct sizes.  Workgroups: every one of them zeroes and flushes a 32 KB LDS histogram,
// and the dense ids are a fraction of the voxels.  meta != nullptr: the sizes were ranked on the device (glszm_rank_kernel),
// k, nsmall and nlarge come from there (kcols bounds k) and the rows of `out` are kstride apart.
int fill_compact_launch(const ZoneState &st, hipStream_t s, const int32_t *image, int Ng, int k, int kcols, const int *large_sorted,
                        double *out, int *err, const int *meta, int kstride) {
  const ZoneArgs z = zone_args(st);
  const int RL = Ng <= 8192 ? std::max(1, std::min(kcols, 8192 / Ng)) : 0;
  hipLaunchKernelGGL(glszm_fill_compact_kernel, dim3(std::min(glszm_grid(st.g.n), 2048u)), dim3(256), sizeof(unsigned) * Ng * RL, s,
                     st.g.n, (const int *)z.labels, z.sizes, image, Ng, k, RL, (const int *)st.small_rank, meta ? 0 : st.nsmall,
                     large_sorted, meta ? 0 : st.nlarge, out, err, z.parent, z.rootctl, meta, kstride, z.tinfo);
  return check_launch("glszm_fill_compact_kernel");
}

// zones, ranking of the distinct sizes, compact fill, features and verdict of one segment-mode volume, enqueued on s, into out_d / empty_d
int features_launches(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, const int *angles, int Na,
                      int Ng, int Ns, double *out_d, int *empty_d) {
  PRAD_TRY(glszm_zones_enqueue(c, s, g, image, mask, angles, Na, Ng));
  ZoneState &st = zone_state();
  // distinct sizes sum to at most n voxels, so there are fewer than sqrt(2 n) + 1 of them
  const int kcap = (int)std::min<long long>(g.n, (long long)std::sqrt(2.0 * (double)g.n) + 2);
  int *stats = nullptr, *flags_d = nullptr, *large_sorted = nullptr, *meta = nullptr, *err = nullptr;
  double *jv = nullptr, *P = nullptr;
  PRAD_TRY(c.get<int>("glszm_stats", 8, &stats));
  PRAD_TRY(c.get<int>("flags", 4, &flags_d));
  PRAD_TRY(c.get<int>("glszm_small_rank", PRAD_SMALL_SIZES, &st.small_rank));
  PRAD_TRY(c.get<int>("glszm_large_sorted", PRAD_RANK_LARGE + 1, &large_sorted));
  PRAD_TRY(c.get<int>("glszm_meta", 8, &meta));
  PRAD_TRY(c.get<int>("glszm_err", 4, &err));
  PRAD_TRY(c.get<double>("glszm_jvals", (size_t)kcap, &jv));
  PRAD_TRY(c.get<double>("glszm_compact", (size_t)Ng * kcap, &P));
  PRAD_TRY(ZeroBatch().add(err, sizeof(int) * 4).add(P, sizeof(double) * (size_t)Ng * kcap).launch(s));
  {
    Timed t(c, "glszm", s);
    hipLaunchKernelGGL(glszm_rank_kernel, dim3(1), dim3(1024), 0, s, (const unsigned *)st.small_bits, (const int *)st.large_list,
                       (const int *)st.large_count, st.large_cap, (const int *)flags_d,
                       (const unsigned long long *)(stats + 2), 2LL * Ns, kcap, st.small_rank, large_sorted, jv, meta);
    PRAD_TRY(check_launch("glszm_rank_kernel"));
    PRAD_TRY(fill_compact_launch(st, s, image, Ng, 0, kcap, large_sorted, P, err, meta, kcap));
  }
  PRAD_TRY(zone_features_launch(c, s, P, Ng, kcap, (long long)kcap, jv, meta + 2, out_d, empty_d));
  hipLaunchKernelGGL(glszm_verdict_kernel, dim3(1), dim3(1), 0, s, (const int *)meta, (const int *)err, out_d + ZM_FEATURES);
  return check_launch("glszm_verdict_kernel");
}

}  // namespace

void prad::glszm_state_invalidate() { zone_state().valid = false; }

extern "C" {

// The route of a segment-mode GLSZM call as ints (the record's order: include/pyradiomics_amd.h).  Host only.
int prad_debug_glszm_route(const int *size, int Nd, const int *angles, int Na, int Ng, int irregular, int *out, int cap) {
  if (!size || !angles || !out || Nd < 1 || Nd > PRAD_MAX_ND || Na < 1 || Ng < 1 || cap < 1) return 0;
  for (int d = 0; d < Nd; d++)
    if (size[d] < 1) return 0;
  GlszmPlan p = glszm_plan(size, Nd, angles, Na, Ng);
  if (irregular) p = glszm_plan_int32(p);
  const int nback = p.tiled() ? p.A.na : 0;
  std::vector<int> r = {(int)p.route, p.mode, p.dims[0], p.dims[1], p.dims[2], (int)p.tiles, nback};
  for (int a = 0; a < nback; a++) r.insert(r.end(), p.A.o[a], p.A.o[a] + 3);
  if ((int)r.size() > cap) return -(int)r.size();
  std::copy(r.begin(), r.end(), out);
  return (int)r.size();
}

int prad_calculate_glszm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                             int Na, int Ng, int Ns, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             long long *nzones, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  Geo g;
  PRAD_TRY(make_geo(size, Nd, &g));
  if (!image || !mask || !angles || Na < 1 || Ng < 1 || Nvox < 1) return fail(PRAD_E_ARG, "bad GLSZM arguments");
  hipStream_t s = (hipStream_t)stream;
  PRAD_TRY(c.begin_call(s));
  int rc = glszm_zones(c, s, g, image, mask, angles, Na, Ng, Ns, Nvox, voxels, kernelRadius, force2Ddim, nzones);
  PRAD_TRY(c.end_call(s));
  PRAD_HIP(hipStreamSynchronize(s));
  return rc;
}

int prad_glszm_features_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                            int Ng, int Ns, double *out, int *empty, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  Geo g;
  PRAD_TRY(make_geo(size, Nd, &g));
  if (!image || !mask || !angles || !out || !empty || Na < 1 || Ng < 1 || Ns < 1) return fail(PRAD_E_ARG, "bad GLSZM arguments");
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = sizeof(double) * (ZM_FEATURES + 1);
  const bool enq = c.deferred && c.in_arena(out, nb) && c.in_arena(empty, sizeof(int));
  const bool direct = enq && Context::zero_copy();        // values, verdict and flag stored straight into the arena
  double *d_out = nullptr;
  PRAD_TRY(c.get<double>("glszm_feat_out", ZM_FEATURES + 4, &d_out));
  int *d_empty = reinterpret_cast<int *>(d_out + ZM_FEATURES + 2);
  PRAD_TRY(c.begin_call(s));
  const int rc = features_launches(c, s, g, image, mask, angles, Na, Ng, Ns, direct ? out : d_out, direct ? empty : d_empty);
  PRAD_TRY(c.end_call(s));            // (the call is closed whether or not the launches succeeded)
  if (rc != PRAD_OK) return rc;
  c.last_path = "glszm-unionfind";
  if (direct) return PRAD_OK;
  if (enq) {
    PRAD_HIP(hipMemcpyAsync(out, d_out, nb, hipMemcpyDeviceToHost, s));
    PRAD_HIP(hipMemcpyAsync(empty, d_empty, sizeof(int), hipMemcpyDeviceToHost, s));
    return PRAD_OK;
  }
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned("glszm_feat_pin", sizeof(double) * (ZM_FEATURES + 4), &pin));
  PRAD_HIP(hipMemcpyAsync(pin, d_out, sizeof(double) * (ZM_FEATURES + 3), hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  memcpy(out, pin, nb);
  memcpy(empty, (const char *)pin + sizeof(double) * (ZM_FEATURES + 2), sizeof(int));
  const int verdict = (int)out[ZM_FEATURES];
  if (verdict & 2) return fail(PRAD_E_INDEX, "GLSZM: zone list would overflow the reference's Ns-sized scratch (Ns=%d)", Ns);
  if (verdict) return fail(PRAD_E_UNSUPPORTED, "GLSZM features: the device-side ranking declined (verdict %d); use prad_calculate_glszm_dev", verdict);
  return PRAD_OK;
}

int prad_fill_glszm_dev(double *glszm, int Nvox, int Ng, int maxRegion, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!glszm || Ng < 1 || maxRegion < 1) return fail(PRAD_E_ARG, "bad fill_glszm arguments");
  hipStream_t s = (hipStream_t)stream;
  const ZoneState *st = live_state(c, "prad_fill_glszm");
  if (!st) return PRAD_E_ARG;
  if (Nvox != st->nvox) return fail(PRAD_E_ARG, "fill_glszm: Nvox=%d but the zone list holds %d kernels", Nvox, st->nvox);
  int *err = nullptr;
  PRAD_TRY(c.get<int>("glszm_err", 4, &err));
  PRAD_HIP(hipMemsetAsync(err, 0, sizeof(int) * 4, s));
  PRAD_HIP(hipMemsetAsync(glszm, 0, sizeof(double) * (size_t)Nvox * Ng * maxRegion, s));
  if (st->segment()) {
    const ZoneArgs z = zone_args(*st);
    const int RL = Ng <= 8192 ? std::max(1, std::min(maxRegion, 8192 / Ng)) : 0;
    hipLaunchKernelGGL(glszm_fill_segment_kernel, dim3(std::min(glszm_grid(st->g.n), 2048u)), dim3(256), sizeof(unsigned) * Ng * RL, s,
                       st->g.n, (const int *)z.labels, z.sizes, st->image, Ng, maxRegion, RL, glszm, err, z.parent, z.rootctl, z.tinfo);
    PRAD_TRY(check_launch("glszm_fill_segment_kernel"));
  } else {
    const long long threads = (long long)st->nvox * st->vox.boxmax;
    hipLaunchKernelGGL(glszm_fill_voxel_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, st->nvox, st->vox.boxmax,
                       st->vox.zones, st->vox.zone_count, Ng, maxRegion, glszm, err);
    PRAD_TRY(check_launch("glszm_fill_voxel_kernel"));
  }
  return fill_verdict(c, s, err);
}

// distinct zone sizes of the preceding segment-mode phase-1 call, ascending, to the host; the size -> column map
// stays on the device for prad_fill_glszm_compact_dev
int prad_glszm_sizes(int *sizes_host, int cap) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  ZoneState *stp = live_state(c, "prad_glszm_sizes");
  if (!stp) return PRAD_E_ARG;
  ZoneState &st = *stp;
  if (!st.segment()) return fail(PRAD_E_UNSUPPORTED, "prad_glszm_sizes: segment mode only");
  if (!sizes_host || cap < 1) return fail(PRAD_E_ARG, "prad_glszm_sizes: bad buffer");
  hipStream_t s = c.own_stream;
  std::vector<unsigned> bits(PRAD_SMALL_SIZES / 32);
  int nl = 0;
  PRAD_HIP(hipMemcpyAsync(bits.data(), st.small_bits, PRAD_SMALL_SIZES / 8, hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipMemcpyAsync(&nl, st.large_count, sizeof(int), hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  if (nl > st.large_cap) return fail(PRAD_E_ARG, "prad_glszm_sizes: internal list overflow (%d > %d)", nl, st.large_cap);
  std::vector<int> large((size_t)nl);
  if (nl) {
    PRAD_HIP(hipMemcpyAsync(large.data(), st.large_list, sizeof(int) * nl, hipMemcpyDeviceToHost, s));
    PRAD_HIP(hipStreamSynchronize(s));
    std::sort(large.begin(), large.end());
    large.erase(std::unique(large.begin(), large.end()), large.end());
  }
  std::vector<int> rank(PRAD_SMALL_SIZES, -1);
  int k = 0;
  for (int sz = 0; sz < PRAD_SMALL_SIZES; sz++)
    if (bits[sz >> 5] & (1u << (sz & 31))) {
      if (k < cap) sizes_host[k] = sz;
      rank[sz] = k++;
    }
  const int nsmall = k;
  for (int v : large) {
    if (k < cap) sizes_host[k] = v;
    k++;
  }
  if (k > cap) return fail(PRAD_E_ARG, "prad_glszm_sizes: %d distinct sizes exceed capacity %d", k, cap);
  int *large_d = nullptr;
  PRAD_TRY(c.get<int>("glszm_small_rank", PRAD_SMALL_SIZES, &st.small_rank));
  PRAD_TRY(c.get<int>("glszm_large_sorted", large.size() + 1, &large_d));
  PRAD_HIP(hipMemcpyAsync(st.small_rank, rank.data(), sizeof(int) * PRAD_SMALL_SIZES, hipMemcpyHostToDevice, s));
  if (!large.empty())
    PRAD_HIP(hipMemcpyAsync(large_d, large.data(), sizeof(int) * large.size(), hipMemcpyHostToDevice, s));
  PRAD_HIP(hipStreamSynchronize(s));
  st.nsizes = k;
  st.nsmall = nsmall;
  st.nlarge = (int)large.size();
  return k;
}

int prad_fill_glszm_compact_dev(double *glszm, int Ng, int k, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!glszm || Ng < 1 || k < 0) return fail(PRAD_E_ARG, "bad fill_glszm_compact arguments");
  hipStream_t s = (hipStream_t)stream;
  const ZoneState &st = zone_state();
  if (!st.valid || st.device != c.device || !st.segment() || st.nsizes < 0)
    return fail(PRAD_E_ARG, "prad_fill_glszm_compact without a preceding prad_glszm_sizes");
  if (k != st.nsizes) return fail(PRAD_E_ARG, "fill_glszm_compact: k=%d but %d distinct sizes were found", k, st.nsizes);
  c.last_variant = glszm_route_name(st.route);
  int *err = nullptr, *large_d = nullptr;
  PRAD_TRY(c.get<int>("glszm_err", 4, &err));
  PRAD_TRY(c.get<int>("glszm_large_sorted", (size_t)st.nlarge + 1, &large_d));
  PRAD_TRY(ZeroBatch().add(err, sizeof(int) * 4).add(glszm, sizeof(double) * (size_t)Ng * std::max(k, 1)).launch(s));
  if (k) PRAD_TRY(fill_compact_launch(st, s, st.image, Ng, k, k, large_d, glszm, err, nullptr, 0));
  return fill_verdict(c, s, err);
}

long long prad_glszm_zones(int v, int *tempData, long long capacity_pairs) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  ZoneState *stp = live_state(c, "prad_glszm_zones");
  if (!stp) return PRAD_E_ARG;
  ZoneState &st = *stp;
  if (!tempData || v < 0 || v >= st.nvox) return fail(PRAD_E_ARG, "prad_glszm_zones: bad kernel index or NULL buffer");
  hipStream_t s = c.own_stream;
  long long count = 0;
  int *pairs = nullptr;
  if (st.model == ZONES_VOXEL) {
    int cnt = 0;
    PRAD_HIP(hipMemcpy(&cnt, st.vox.zone_count + v, sizeof(int), hipMemcpyDeviceToHost));
    count = cnt;
    if (count > capacity_pairs) return fail(PRAD_E_ARG, "prad_glszm_zones: %lld zones exceed capacity %lld", count, capacity_pairs);
    PRAD_TRY(c.get<int>("glszm_pairs", (size_t)count * 2 + 2, &pairs));
    if (count) {
      hipLaunchKernelGGL(glszm_gather_zones_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, st.nvox, v,
                         (int)count, st.vox.zones, pairs);
      PRAD_TRY(check_launch("glszm_gather_zones_kernel"));
    }
  } else {
    count = st.nzones;
    if (count > capacity_pairs) return fail(PRAD_E_ARG, "prad_glszm_zones: %lld zones exceed capacity %lld", count, capacity_pairs);
    const long long n = st.g.n, nblocks = (n + PRAD_ZL_BLOCK - 1) / PRAD_ZL_BLOCK;
    unsigned *counts = nullptr;
    unsigned long long *offsets = nullptr;
    PRAD_TRY(c.get<unsigned>("glszm_bcounts", (size_t)nblocks, &counts));
    PRAD_TRY(c.get<unsigned long long>("glszm_boffsets", (size_t)nblocks, &offsets));
    PRAD_TRY(c.get<int>("glszm_pairs", (size_t)count * 2 + 2, &pairs));
    const int *roots = st.vol.labels;          // labels[v] == v at the first voxel v of every zone
    const unsigned *vsizes = st.vol.sizes;     // ... and the zone's size at the same index
    if (st.model == ZONES_DENSE) {
      // vid[] has done its work (the unions are over) -- its array becomes the view this scan needs: v at the first voxel v of
      // every zone, -1 elsewhere, the zone sizes in a voxel-indexed scratch array
      DenseZones &d = st.dense;
      int *zmin = nullptr;
      unsigned *zsz = nullptr;
      PRAD_TRY(c.get<int>("glszm_zmin", d.idcap, &zmin));
      PRAD_TRY(c.get<unsigned>("glszm_zsz", (size_t)n, &zsz));
      if (!d.published) {                       // (d.vid is vid[] only until the first call)
        PRAD_HIP(hipMemsetAsync(zmin, 0x7f, sizeof(int) * d.idcap, s));
        hipLaunchKernelGGL(glszm_zmin_kernel, dim3(2048), dim3(256), 0, s, n, (const int *)d.vid, (const int *)d.parent, zmin);
        d.published = true;
      }
      PRAD_HIP(hipMemsetAsync(d.vid, 0xff, sizeof(int) * (size_t)n, s));
      hipLaunchKernelGGL(glszm_publish_kernel, dim3(1024), dim3(256), 0, s, (const int *)d.rootctl, (const int *)d.parent,
                         (const unsigned *)d.tsize, (const int *)zmin, d.vid, zsz);
      PRAD_TRY(check_launch("glszm_publish_kernel"));
      roots = d.vid;
      vsizes = zsz;
    }
    hipLaunchKernelGGL(glszm_root_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, n, roots, counts);
    PRAD_TRY(check_launch("glszm_root_count_kernel"));
    hipLaunchKernelGGL(glszm_scan_kernel, dim3(1), dim3(1024), 0, s, nblocks, counts, offsets);
    PRAD_TRY(check_launch("glszm_scan_kernel"));
    hipLaunchKernelGGL(glszm_root_scatter_kernel, dim3((unsigned)nblocks), dim3(64), 0, s, n, roots, vsizes, st.image, offsets, pairs);
    PRAD_TRY(check_launch("glszm_root_scatter_kernel"));
  }
  if (count) PRAD_HIP(hipMemcpyAsync(tempData, pairs, sizeof(int) * 2 * count, hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  tempData[count * 2] = -1;  // cmatrices.c:276
  return count;
}

}  // extern "C"
