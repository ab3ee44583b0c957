// prad_glszm_plan.h -- which kernels label the zones of a segment-mode GLSZM call: a pure function of (size, Nd, angles, Na, Ng).
// No Context, no HIP call: prad_debug_glszm_route records its result and tests/test_glszm_route_plan.py holds it to a
// restatement of the rules below, without a device.
//
// The volume is embedded in 3-D (leading extents 1).  An offset is BACKWARD when its linear index in the embedded volume is
// negative; only backward offsets are kept (the pair of a forward one is handled from its other end).
//   tiled   Nd <= 3, Na <= 64, every offset component in {-1, 0, 1}, at most 32 backward offsets
//   mode    1 with 13 backward offsets (the full 26-neighbourhood), 2 with 4 backward offsets that all have dz == 0 (the full
//           in-plane 8-neighbourhood), otherwise 0: with a full neighbourhood the redundancy rules of the tile kernels apply
//   dense   tiled, mode != 0 and 1 <= Ng <= 255: the levels fit the byte pack
// Routes: dense 26 / dense 8 (kernels_glszm_dense.h); int32 tiles (glszm_tile_kernel) with the border kernel of the mode -- full
// 26, full 8 or the offset table; the label volume for everything that is not tiled (kernels_glszm_labels.h).  A masked level
// outside 1..Ng, found by the pack of a dense call, reruns the call as the int32 tiles of the same mode (glszm_plan_int32).
#pragma once

// the tile of the tiled routes, in voxels
#define PRAD_TZ 8
#define PRAD_TY 8
#define PRAD_TX 64
#define PRAD_TVOX (PRAD_TZ * PRAD_TY * PRAD_TX)

namespace prad {

struct Offsets3 {
  int na;
  signed char o[32][4];   // backward neighbours only (linear offset < 0), embedded in 3-D
};

// (GLSZM_VOXEL: voxel mode is not planned here, only named for prad_last_variant())
enum GlszmRoute { GLSZM_DENSE26, GLSZM_DENSE8, GLSZM_TILES_FULL26, GLSZM_TILES_FULL8, GLSZM_TILES_OFFSETS, GLSZM_LABEL_VOLUME, GLSZM_VOXEL };
inline const char *glszm_route_name(GlszmRoute r) {
  static const char *const names[] = {"dense26", "dense8", "tiles-full26", "tiles-full8", "tiles-offsets", "label-volume", "voxel-flood"};
  return names[r];
}

struct GlszmPlan {
  GlszmRoute route;
  int mode;          // 0 / 1 / 2, see above (0 for the label volume)
  Offsets3 A;        // meaningful on the tiled routes
  int dims[3];       // the 3-D-embedded extents (Nz, Ny, Nx)
  long long tiles;   // workgroups of the tile kernel; 0 for the label volume
  bool dense() const { return route == GLSZM_DENSE26 || route == GLSZM_DENSE8; }
  bool tiled() const { return route != GLSZM_LABEL_VOLUME && route != GLSZM_VOXEL; }
};

inline GlszmPlan glszm_plan(const int *size, int Nd, const int *angles, int Na, int Ng) {
  GlszmPlan p;
  p.route = GLSZM_LABEL_VOLUME;
  p.A.na = p.mode = 0;
  p.tiles = 0;
  p.dims[0] = p.dims[1] = p.dims[2] = 1;
  if (Nd > 3 || Na > 64) return p;
  for (int d = 0; d < Nd; d++) p.dims[3 - Nd + d] = size[d];
  for (int a = 0; a < Na; a++) {
    int o[3] = {0, 0, 0};
    for (int d = 0; d < Nd; d++) o[3 - Nd + d] = angles[a * Nd + d];
    if (o[0] < -1 || o[0] > 1 || o[1] < -1 || o[1] > 1 || o[2] < -1 || o[2] > 1) return p;
    const long long lin = ((long long)o[0] * p.dims[1] + o[1]) * p.dims[2] + o[2];
    if (lin >= 0) continue;                 // forward neighbour: its pair is handled from the other end
    if (p.A.na >= 32) return p;
    for (int d = 0; d < 3; d++) p.A.o[p.A.na][d] = (signed char)o[d];
    p.A.o[p.A.na][3] = 0;
    p.A.na++;
  }
  if (p.A.na == 13) p.mode = 1;
  else if (p.A.na == 4) {
    p.mode = 2;
    for (int a = 0; a < 4; a++)
      if (p.A.o[a][0] != 0) p.mode = 0;
  }
  p.tiles = (long long)((p.dims[0] + PRAD_TZ - 1) / PRAD_TZ) * ((p.dims[1] + PRAD_TY - 1) / PRAD_TY) *
            ((p.dims[2] + PRAD_TX - 1) / PRAD_TX);
  const bool bytes = p.mode != 0 && Ng >= 1 && Ng <= 255;
  p.route = p.mode == 1 ? (bytes ? GLSZM_DENSE26 : GLSZM_TILES_FULL26)
          : p.mode == 2 ? (bytes ? GLSZM_DENSE8 : GLSZM_TILES_FULL8) : GLSZM_TILES_OFFSETS;
  return p;
}

// the plan a dense call is rerun with when its pack found an irregular level: the int32 tiles of the same mode
inline GlszmPlan glszm_plan_int32(GlszmPlan p) {
  if (p.dense()) p.route = p.mode == 1 ? GLSZM_TILES_FULL26 : GLSZM_TILES_FULL8;
  return p;
}

}  // namespace prad
