// prad_internal.h -- what the host units of the texture engine share: functions that one of prad_api.hip, prad_glszm.hip and
// prad_features.hip defines and another of them, or prad_image.hip (the case pipeline's queues and launcher, no kernel of its
// own), calls.  Nothing here belongs to the C ABI: that is include/pyradiomics_amd.h.
#pragma once
#include "prad_runtime.h"

#define ZM_FEATURES 16   // ZM_COUNT of kernels_features.h (static_assert there)

namespace prad {
#pragma GCC visibility push(hidden)

constexpr int kMaxSweepAngles = 16;   // PRAD_MAX_SWEEP of kernels_sweep.h (static_assert in prad_api.hip)

// angle enumeration (cmatrices.c:756-892)
int angle_count(const int *size, const int *distances, int Nd, int Ndist, int bidirectional, int f2d);
int angle_build(const int *size, const int *distances, int Nd, int Ndist, int f2d, int Na, int *angles);

// GLCM and/or GLRLM, and GLDM + NGTDM from one pass, of device arrays on stream s (the entry points' common half)
int texture_pairs_runs(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na, int Ng,
                       int Nr, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, double *glcm, double *glrlm,
                       hipStream_t s);
int texture_gldm_ngtdm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na, int Ng,
                       int alpha, double *gldm, double *ngtdm, hipStream_t s);

// the byte-packed copy of a derived image that its neighbourhood pass and its GLSZM share (the pack kernel and the record of
// the copy belong to prad_api.hip's kernel headers)
int image_shared_pack(Context &c, const int32_t *levels, const uint8_t *mask, long long n, int NX, int Ng, int ticket,
                      hipStream_t s);
void image_shared_pack_clear();

// prad_glszm.hip's dense routes: the byte pack of a whole volume on s, bracketed as "pack", or the shared pack above when it is
// this image's; flags_d[0] != 0: a masked level outside [1, Ng]
int glszm_byte_pack(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, int Ng, int *flags_d,
                    uint8_t **levels);
// prad_glszm.hip: the zones of the last GLSZM call live in the workspace and go with it (prad_release_workspace)
void glszm_state_invalidate();

#pragma GCC visibility pop

// prad_features.hip, for prad_glszm_features_dev: launch only, the columns were found on the device (default visibility, as defined)
int zone_features_launch(Context &c, hipStream_t s, const double *P, int Ni, int Njcap, long long stride_i,
                         const double *jvals_d, const int *nj_dev, double *out_d, int *empty_d);
}  // namespace prad

// prad_image.hip: the image queues' streams and events go with the workspace (prad_release_workspace).  C linkage and default
// visibility: the library has always exported this name, and its list of exported symbols stays as it was.
extern "C" void release_image_queues(void);
