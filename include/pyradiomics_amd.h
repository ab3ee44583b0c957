/*
 * pyradiomics_amd.h -- C ABI of the MI355X (gfx950) texture-matrix engine.
 *
 * This is the drop-in boundary for pyradiomics' native operator layer.  It replaces
 *   - the eight C prototypes of radiomics/src/cmatrices.h:1-8, and
 *   - the per-voxel driver loops of the CPython wrapper radiomics/src/_cmatrices.c
 *     (set_bb :1120-1147 and the `for v in Nvox` loops :203-222, :355-377, :552-570, :700-718,
 *     :850-868), which are folded into the calls below so that a whole voxel batch is ONE launch.
 * The Python face `radiomics.cMatrices` (radiomics/__init__.py:343-349) is restored on top of this
 * ABI by pyradiomics_amd/cmatrices.py with ctypes; see INTEGRATION.md for the binding a reference
 * maintainer would add.
 *
 * Conventions (all functions):
 *   - plain pointers and ints only; no exceptions cross the boundary; thread-safe per device.
 *   - `image` is int32 [size[0]]...[size[Nd-1]] C-contiguous, `mask` is uint8/bool of the same shape
 *     (what _cmatrices.c:1023-1085 coerces its inputs to).  1 <= Nd <= PRAD_MAX_ND.
 *   - voxel mode: `voxels` is int32 [Nd][Nvox] (np.where layout, _cmatrices.c:1087-1118); kernel v covers
 *     centre +- kernelRadius clamped to the array, collapsed in force2Ddim.  Segment mode: voxels=NULL,
 *     Nvox=1, box = whole array.  force2Ddim = -1 when force2D is off (_cmatrices.c:126).
 *   - outputs are caller-allocated float64 arrays in the reference's layouts; they need NOT be
 *     pre-zeroed (the reference memsets them itself, e.g. _cmatrices.c:185).
 *   - return value: PRAD_OK (1) on success; PRAD_INDEX_ERROR (0) where the reference's core returns 0
 *     ("index out of range", surfaced by the wrapper as IndexError, _cmatrices.c:219,566,714,864);
 *     negative PRAD_E_* for everything else; prad_last_error() gives the message.
 *   - the `_dev` variants take DEVICE pointers for image/mask/voxels/outputs and a hipStream_t (as
 *     void*); they enqueue on that stream and synchronise it before returning the status.
 *     The host variants stage through the library's per-device workspace.
 */
#ifndef PYRADIOMICS_AMD_H
#define PYRADIOMICS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRAD_MAX_ND 8

#define PRAD_OK 1
#define PRAD_INDEX_ERROR 0
#define PRAD_E_ARG (-1)         /* bad argument (NULL pointer, Nd out of range, kernelRadius <= 0 with voxels...) */
#define PRAD_E_HIP (-2)         /* HIP runtime failure; message in prad_last_error() */
#define PRAD_E_NOMEM (-3)       /* device or host allocation failed */
#define PRAD_E_UNSUPPORTED (-4) /* valid for the reference but not implemented here (stated in the message) */
#define PRAD_E_INDEX (-5)       /* GLSZM phase 1 only: the reference's calculate_glszm would return -1 (scratch sized by
                                   Ns exhausted, cmatrices.c:174,226,245,274) -> IndexError in the wrapper */

/* ---- runtime ---------------------------------------------------------------------------------- */
const char *prad_version(void);
const char *prad_last_error(void);       /* thread-local, valid until the next failing call */
int prad_device_count(void);             /* number of visible HIP devices (0 if none) */
int prad_set_device(int device);         /* selects the device used by this thread's later calls */
int prad_get_device(void);
/* The library keeps grow-only scratch buffers per calling thread and device (packed levels, accumulators, union-find
 * labels, staging copies of host inputs ...) so that repeated calls of the same shape allocate nothing.
 * prad_workspace_bytes: device bytes currently held by the calling thread; prad_release_workspace: free them (and
 * the pinned host buffers); any pending two-phase GLSZM state is dropped. */
long long prad_workspace_bytes(void);
int prad_release_workspace(void);
/* name of the code path taken by this thread's last calculate_* call ("sweep", "generic", ...);
 * lets tests assert that the fast kernels (not a fallback) produced a result. */
const char *prad_last_path(void);
/* which sweep kernels the plan of this thread's last GLCM / GLRLM call chose: "fw" (fixed window, fused table: <= 36 grey
 * levels, rows of 65..1024 voxels), "fw2" (fixed window, two tables, 16-bit levels: 40 .. 170 levels, rows of 65..512), "lines" (wrapped lines);
 * after prad_label_census*: "census-lds" or "census-global". */
const char *prad_last_variant(void);
/* Total device time (ms, HIP events on the work stream) of this thread's last calculate_* call, and
 * the time of its dominant kernel family; used by bench.py for the roofline figure. */
double prad_last_device_ms(void);
double prad_last_kernel_ms(const char *kernel_family);
/* Accumulated timing over many calls (the per-call figures above need the call to have finished, i.e. one host
 * synchronisation per call).  prad_timing_begin: start keeping the event brackets of every following call of this
 * thread; prad_timing_ms: sum of the brackets of a kernel family (NULL: whole calls) since then, in ms -- synchronises
 * on the last recorded event; prad_timing_calls: calls recorded; prad_timing_end: stop and drop the records.
 * prad_timing_begin_only(family): as prad_timing_begin, but ONLY the launches of that kernel family are bracketed (no call
 * brackets either) -- two event records per call instead of ten: a timed loop that wants the duration of its dominant
 * kernel without paying for the rest (each record costs the stream 3 - 6 us; bench.py).  prad_timing_count(family): how
 * many brackets of the family were recorded (NULL: calls). */
int prad_timing_begin(void);
int prad_timing_begin_only(const char *kernel_family);
int prad_timing_count(const char *kernel_family);
double prad_timing_ms(const char *kernel_family);
int prad_timing_calls(void);
int prad_timing_end(void);
/* Deferred mode for the device-pointer GLCM / GLRLM entry points (segment mode): with on != 0 a call only ENQUEUES its
 * kernels on the caller's stream and returns without synchronising the host, so consecutive volumes pipeline on the
 * GPU.  The one thing the host learns late is whether a volume held masked levels outside [1, Ng] (which the
 * synchronous call answers by re-running on the exact generic kernels): every deferred call latches that into a sticky
 * device flag; prad_deferred_status synchronises the stream, returns PRAD_OK, or PRAD_E_DEFERRED if any deferred call
 * since the last query saw such levels (its outputs are then undefined: repeat that call synchronously), and clears
 * the flag.  Calls the sweep kernels cannot serve (voxel mode, Nd > 3, ...) run synchronously as before.
 * Lanes: deferred whole-volume calls are dealt round-robin onto `n` internal streams (default 2, environment
 * PRAD_LANES; 1 = everything stays on the caller's stream), each with its own workspace and each waiting for the work
 * queued on the caller's stream at the time of the call, so the kernels of consecutive volumes share the GPU.  The
 * caller's stream does NOT wait for a lane: inputs and outputs of a deferred call belong to the library until
 * prad_deferred_status returns (it synchronises the stream and every lane).
 * Pipeline (the default deferred mode; prad_set_deferred_mode(0) or PRAD_DEFERRED_MODE=lanes selects the lanes):
 * deferred whole-volume calls stay on the caller's stream (but see "Twin pipelines" below) and form a two-stage pipeline -- call N launches the walks of
 * volume N-1 with the PACK of volume N riding in the same launch as a side job of the walking waves (the pack is
 * HBM-bound, the walk issue-bound: the pack's memory time disappears), then finalizes volume N-1.  Volume N is walked by
 * the next deferred call, or by prad_deferred_join / prad_deferred_status, which flush the pipeline.  As with the lanes,
 * inputs and outputs of a deferred call belong to the library until one of those two returns.  The pipeline takes the
 * volumes of the fixed-window kernels -- fused table (up to 36 levels) and, since round 5, two tables (40 .. 170 levels;
 * a volume of the other kind than the one before it packs in a launch of its own) -- every other whole-volume call is
 * dealt onto the lanes.
 * Twin pipelines: large volumes (from 2^27 voxels, 512^3; PRAD_PIPE_TWIN=1 forces it for every pipeline volume,
 * PRAD_PIPE_TWIN=0 switches it off) do NOT stay on the caller's stream: they are dealt alternately onto TWO instances of the
 * pipeline, each on an internal stream of its own (the lanes' streams 0 and 1) that waits for the work queued on the caller's
 * stream at the time of the call, each with workspace sets of its own.  Consecutive walk launches are then unordered on the
 * device and fill each other's uneven ends.  The contract is the one above -- inputs and outputs belong to the library until
 * prad_deferred_status or prad_deferred_join returns; both cover both pipelines -- with a volume's outputs written two calls
 * later than on one pipeline.  Two in-flight calls that name the same output buffer end with the later call's values, as on
 * one stream.  The brackets of prad_timing_* are recorded on the stream a launch goes to; with overlapping launches a bracket's
 * duration is no kernel speed (take those with PRAD_PIPE_TWIN=0). */
#define PRAD_E_DEFERRED (-6)
int prad_set_deferred(int on);
int prad_set_lanes(int n);                 /* 0 = default; returns PRAD_E_ARG outside [0, 4] */
int prad_set_deferred_mode(int mode);      /* 1 pipeline, 0 lanes, -1 environment default (PRAD_DEFERRED_MODE); flushes */
/* makes `stream` wait ON THE DEVICE for every deferred call issued so far (no host synchronisation): afterwards work
 * queued on `stream` may read the outputs of those calls; the levels verdict still needs prad_deferred_status */
int prad_deferred_join(void *stream);
int prad_deferred_status(void *stream);
/* queues a copy of the sticky verdict word into `flag` (an int inside the result arena) on `stream`: a caller that waits
 * on an EVENT recorded after this call -- not on the whole stream, so that work queued later keeps running -- reads
 * *flag != 0 as "a deferred call before the mark saw levels outside [1, Ng]" (then prad_deferred_status clears it) */
int prad_deferred_mark(int *flag, void *stream);
/* Result arena + enqueue-only feature calls (the case pipeline: every matrix and feature kernel of one derived image is
 * queued before the host waits once).  prad_result_alloc hands out pinned host memory from a per-thread ring of 4 MiB
 * (64-byte aligned; at most 1 MiB per allocation; an allocation stays untouched until 4 MiB more have been handed out).
 * In deferred mode (prad_set_deferred(1)):
 *  - prad_calculate_gldm_dev / prad_calculate_ngtdm_dev in segment mode only enqueue their kernels; a level outside
 *    [1, Ng] under the mask is latched like the GLCM / GLRLM verdict (prad_deferred_status -> PRAD_E_DEFERRED);
 *  - prad_glcm_features_dev, prad_zone_matrix_features_dev, prad_ngtdm_features_dev and prad_glcm_mcc_dev whose output
 *    pointers lie INSIDE the arena enqueue their kernels and the device-to-host copies into those pointers and return:
 *    the values are valid once the stream has been synchronised (prad_deferred_status, or an event recorded after the
 *    call).  The arena is mapped host memory: the formula kernels store their few values straight into it (no copy
 *    operation in the stream; PRAD_ZERO_COPY=0 restores device buffer + copy).  prad_glcm_mcc_dev then needs room for Na + 1 doubles: out[Na] != 0 says that more than 64 grey levels
 *    occurred (the synchronous call's PRAD_E_UNSUPPORTED) and out[0..Na) is void.
 * With outputs outside the arena these calls stay synchronous.  All calls of one pipeline go to ONE stream (the
 * workspace buffers are recycled in stream order).  No reference analogue (the reference computes the formulas in numpy
 * from host matrices: glcm.py, glrlm.py, ...). */
int prad_result_alloc(size_t bytes, void **out);
/* Workspace set of the calling thread (0 = default, 1..7): the library recycles named scratch buffers in stream order, so
 * a thread that issues calls on a SECOND stream concurrently selects another set for them (and switches back).  The
 * case pipeline queues its enqueue-only classes on a side stream under set 1 while first order / GLSZM run on the main
 * stream under set 0. */
int prad_set_workspace(int id);
/* One derived image, every class, one call: the enqueue half of the case pipeline in native code.  levels / mask: DEVICE
 * (discretised image, ROI); raw: DEVICE undiscretised image of dtype raw_dtype (first order; NULL without that class);
 * Ns = ROI voxels; classes = sum of PRAD_IMG_* (PRAD_IMG_MCC with PRAD_IMG_GLCM adds the MCC); distance-1 neighbourhoods,
 * force2Ddim as elsewhere.  Queues, without waiting: GLCM + GLRLM (one sweep), their formulas and the MCC, GLDM + NGTDM (one
 * pass over the neighbourhoods) and their formulas on an internal stream, GLSZM on a second, first order on a third -- each
 * stream waits for the work queued on `stream` so far and has its own workspace set -- and a verdict mark + event behind
 * each.  *results: one block of the result arena; layout[k] (int[16]) = offset of part k in doubles, -1 = not asked for or
 * declined by the device route (the caller then computes that class on its own):
 *   0 GLCM values [Na][23], 1 GLCM "angle empty" flags (int [Na]), 2 MCC [Na] + verdict, 3 GLRLM values [Na][16], 4 flags,
 *   5 GLDM values [16], 6 flag, 7 NGTDM values [5], 8 GLSZM values [16] + verdict, 9 flag, 10 first order [15] + verdict;
 *   layout[11] = Na, layout[12] = doubles in the block.
 * prad_image_wait(ticket) waits for the image's work only (later images keep running; up to 4 images may be in flight per
 * thread) and returns PRAD_OK, or PRAD_E_DEFERRED when a queued call saw levels outside [1, Ng] (values void).  Inputs
 * must stay alive until then.  No reference analogue (base.py:181-198 evaluates class after class on the host). */
#define PRAD_IMG_GLCM 1
#define PRAD_IMG_GLRLM 2
#define PRAD_IMG_GLDM 4
#define PRAD_IMG_NGTDM 8
#define PRAD_IMG_GLSZM 16
#define PRAD_IMG_FIRSTORDER 32
#define PRAD_IMG_MCC 64
int prad_image_enqueue_dev(const int32_t *levels, const uint8_t *mask, const void *raw, int raw_dtype, const int *size,
                           int Nd, int Ng, long long Ns, int classes, int symmetric, int alpha, int force2Ddim,
                           double voxelArrayShift, double **results, int *layout, int *ticket, void *stream);
int prad_image_wait(int ticket);
/* prad_image_enqueue_dev issued from a LAUNCHER thread that belongs to the calling thread (created on first use; it has a
 * workspace, result arena, side streams and tickets of its own).  One derived image is ~65 launches, copies and fills: 0.25 ms
 * of host time per image on a path that is bound by its host thread (featureextractor.py:371-395 + base.py:181-198 in the
 * reference are that thread too).  prad_image_submit copies the arguments and returns at once (*job: slot of up to four in
 * flight per thread); the side streams wait for what was queued on `stream` by the time the launcher gets to the job, i.e.
 * at least for everything the caller queued before the call.  prad_image_submit_result blocks until the launcher has ISSUED
 * the job (not until the GPU has run it) and returns prad_image_enqueue_dev's code, result block and layout;
 * prad_image_submit_wait waits for the image's GPU work like prad_image_wait and frees the slot (it must be called exactly
 * once per job, also after a failed submit).  Jobs of one calling thread are issued in order.  prad_image_submit_release:
 * prad_release_workspace on the launcher's context (nothing may be in flight). */
int prad_image_submit(const int32_t *levels, const uint8_t *mask, const void *raw, int raw_dtype, const int *size, int Nd, int Ng,
                      long long Ns, int classes, int symmetric, int alpha, int force2Ddim, double voxelArrayShift, void *stream,
                      int *job);
int prad_image_submit_result(int job, double **results, int *layout);
int prad_image_submit_wait(int job);
int prad_image_submit_release(void);

/* ---- angles: cmatrices.h get_angle_count / build_angles (cmatrices.c:756-892) ------------------- */
/* returns the number of angles, 0 on invalid distance (as the reference) */
int prad_get_angle_count(const int *size, const int *distances, int Nd, int Ndist, int bidirectional,
                         int force2Ddim);
/* returns 0 on success, 1 on invalid distance (as the reference); angles is int32 [Na][Nd] */
int prad_build_angles(const int *size, const int *distances, int Nd, int Ndist, int force2Ddim, int Na,
                      int *angles);

/* ---- debug: the sweep plan of a segment-mode GLCM / GLRLM call (no device call, no launch) ----------------------------
 * Plans for a volume of `size` ([Nd], Nd <= 3 for a plan), the HOST angle list `angles` ([Na][Nd]), Ng levels and Nr run
 * lengths as a real call does -- the environment's switches included -- with `cus` compute units (<= 0: the device's count,
 * 256 without a device).  Writes the plan to out[0 .. cap) as ints and returns how many it wrote; -(the count needed) when
 * cap is too small; 0 for arguments no call accepts.  The record:
 *   ok                                   0: the call takes another route, and the record ends here
 *   Nz Ny Nx  fused fw fw2 fw2_rows
 *   RS RSr RSfw RSfw_rows RS2 RS2r  LONG LONGr LONGfw LONGfw2 LONGfw2r
 *   lds_bytes lds_bytes_rows lds_fw lds_fw_rows lds_fw2 lds_fw2_rows
 *   threads fw_threads fw_rows_threads fwK fw_blocks fw2_copies fw2r_copies fw2r_waves
 *   LPL pitch padw pitch16 vec_rows  skip1 row_slot fw_xblocks
 *   lines.count, then per line angle:    slot NM NU NX du dx sM sU LXc chunks
 *   aset.count, then per angle:          its offset (z, y, x)
 *   has_fwset (fw or fw2), and if 1:     count NX pitch nrows xcd  first_block[17]  xslot xRS xwaves xgpd,
 *                                        then per line angle: slot NM NU du dx sM sU CL pieces chunks dom_kind
 * (64-bit strides and chunk counts are narrowed to int.)  tests/test_sweep_plan.py pins these records. */
int prad_debug_sweep_plan(const int *size, int Nd, const int *angles, int Na, int Ng, int Nr, int want_glcm, int want_glrlm,
                          int cus, int *out, int cap);

/* ---- debug: the launches the deferred GLCM + GLRLM pipeline plans for a script of events (no device call, no launch) ----
 * Replays `nevents` events through a FRESH planner (csrc/prad_pipe_plan.h), not the calling thread's live one, as the
 * executor runs deferred calls through its own.  Writes one record of 13 ints per planned launch to out[0 .. cap) and returns
 * how many ints it wrote; -(the count needed) when cap is too small; 0 when nothing is launched or for NULL arguments.
 * An event is 14 int64:
 *   [0]  type            0 a flush (prad_deferred_join / _status / _mark), 1 a deferred whole-volume call,
 *                        2 the workspace is released (a flush, then nothing is known to be zero any more),
 *                        3 a deferred call that fails behind the choice of its set (arguments no call accepts): it takes a set
 *                          (reads [1], [5], [13] as a call does) and launches nothing of its own
 *   [9]  fin_ride        the switch PRAD_FIN_RIDE as the call or the flush reads it (0 / 1)      -- every type; the rest: calls
 *   [1]  voxels          of the volume (automatic twin from 2^27)
 *   [2]  rows            Nz * Ny: a fused-table volume uses (rows + 3) / 4 words of row flags, a two-table volume none
 *   [3]  acc_words       accumulators + control words of the volume
 *   [4]  kind            0 fused table, 1 two tables, 2 a volume the pipeline does not take (both instances are flushed)
 *   [5]  twin            the switch PRAD_PIPE_TWIN: 1, 0, or -1 = by the voxel count
 *   [6]  stream          the caller's stream, any id (a twin call runs on the instance's internal stream instead)
 *   [7]  rz_id  [8] rz_cap   the row-flag buffer the volume's set has at this call: an opaque non-zero id and its capacity in
 *                        bytes (the caller of the replay decides when the buffer "grows" or is allocated anew)
 *   [10] can_ride        the volume's finalize can ride in a walk launch (plan, PRAD_FINALIZE_ONE, PRAD_FW_XROLE: fin_can_ride)
 *   [11] host_plan_ok    the volume's walk launch can carry a riding job as far as its plan goes (fin_host_ok)
 *   [12] pack_inline_ok  the volume's pack can ride in a walk launch of its kind (pack_inline_ok, PRAD_NO_INLINE_PACK)
 *   [13] outs_overlap    the call's outputs overlap outputs the other instance has in flight (it is flushed first)
 * A record:
 *   event                index of the event that launches it
 *   kind                 0 zero3_kernel, 1 a stand-alone finalize, 2 a walk launch, 3 a stand-alone pack
 *   instance             0 / 1
 *   walk  pack  fin      workspace sets (-1: none).  walk launch: the set it walks, the set whose pack rides in it, the set
 *                        whose finalize rides in it; finalize / pack launch: the set it finishes / packs
 *   job                  walk launch: 1 if it may carry a riding job at all
 *   acc_set acc_words  rz_set rz_words  fl_set fl_words
 *                        the word ranges (accumulators + control words, row flags, flag words; set -1: none) that a
 *                        zero3_kernel launch zeroes, or that the riding job of a walk launch zeroes
 * (word counts are narrowed to int.)  tests/test_pipe_plan.py checks these records against a model of the workspace. */
int prad_debug_pipe_plan(const long long *events, int nevents, int *out, int cap);

/* ---- debug: the route of a segment-mode GLSZM call (no device call, no launch) ------------------------------------------
 * Plans for `size` ([Nd]), the HOST angle list `angles` ([Na][Nd]) and Ng levels as prad_calculate_glszm_dev does
 * (csrc/prad_glszm_plan.h); irregular != 0: the route the call is rerun on when its byte pack finds a masked level outside
 * [1, Ng].  Writes ints to out[0 .. cap), returns their number; -(the number needed) when cap is too small; 0 for arguments no
 * call accepts.  The record:
 *   route      0 dense 26, 1 dense 8, 2 / 3 / 4 int32 tiles with the full-26 / full-8 / offset-table border kernel, 5 label volume:
 *              the prad_last_variant() names "dense26", "dense8", "tiles-full26", "tiles-full8", "tiles-offsets", "label-volume"
 *   mode       1 the full 26-neighbourhood, 2 the full in-plane 8-neighbourhood, 0 neither
 *   Nz Ny Nx   the 3-D-embedded extents (1 1 1 for the label volume of more than three dimensions)
 *   tiles      workgroups of the tile kernel (0: label volume)
 *   nback      backward offsets (0: label volume), then per offset: dz dy dx
 * tests/test_glszm_route_plan.py checks these records against the rules. */
int prad_debug_glszm_route(const int *size, int Nd, const int *angles, int Na, int Ng, int irregular, int *out, int cap);

/* ---- debug: the pairs tier of a segment-mode GLDM / NGTDM call (no device call, no launch) -----------------------------
 * Plans as pairs_neigh does (csrc/prad_neigh_plan.h) for `size` ([Nd]), the HOST angle list `angles` ([Na][Nd]) and Ng levels;
 * ngtdm: 0 GLDM, 1 NGTDM; knobs: bit 0 PRAD_NO_PAIRS, bit 1 PRAD_NGTDM_NO_BOX (the environment is NOT read); cus <= 0: the
 * device's count, 256 without a device.  Writes 15 ints to out[0 .. cap), returns their number; -(the number needed) when cap is
 * too small; 0 for arguments no call accepts.  The record:
 *   applies  variant      the tier takes the call; index into the prad_last_variant() names "none", then "pairs-global",
 *                         "pairs-lds64", "pairs-lds32" each plain, "+box32" and "+box64" (1 + 3 * placement + word)
 *   box narrow  mode      box sums, in 32-bit words; bins 0 global, 1 LDS, 2 LDS as u32 under the grid's voxel cap
 *   lds threads grid  box_grid     LDS bytes, workgroup size and grid of the bin kernel; grid of the box-axis kernels
 *   Nz Ny Nx  rz ry rx    the 3-D-embedded extents; the largest |offset| per axis
 * tests/test_neigh_route_plan.py checks these records against tests/neigh_reference.expected_route and the overflow rule. */
int prad_debug_neigh_plan(const int *size, int Nd, const int *angles, int Na, int Ng, int ngtdm, int knobs, int cus, int *out, int cap);

/* ---- GLCM: calculate_glcm (cmatrices.c:4-92) ---------------------------------------------------- */
/* glcm: float64 [Nvox][Ng][Ng][Na] */
int prad_calculate_glcm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                        const int *angles, int Na, int Ng,
                        int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                        double *glcm);
int prad_calculate_glcm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                            const int *angles, int Na, int Ng,
                            int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                            double *glcm, void *stream);

/* ---- GLRLM: calculate_glrlm (cmatrices.c:299-541) ----------------------------------------------- */
/* glrlm: float64 [Nvox][Ng][Nr][Na] */
int prad_calculate_glrlm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                         const int *angles, int Na, int Ng, int Nr,
                         int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         double *glrlm);
int prad_calculate_glrlm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                             const int *angles, int Na, int Ng, int Nr,
                             int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             double *glrlm, void *stream);

/* ---- GLCM + GLRLM in one call (the headline path: one discretised volume -> both matrices).
 * Same results as the two calls above with the same `angles`; the volume is packed once and every
 * angle is swept once for both matrices.  Either output may be NULL to skip it. ------------------- */
int prad_calculate_glcm_glrlm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                              const int *angles, int Na, int Ng, int Nr,
                              int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                              double *glcm, double *glrlm);
int prad_calculate_glcm_glrlm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                  const int *angles, int Na, int Ng, int Nr,
                                  int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                                  double *glcm, double *glrlm, void *stream);

/* ---- GLDM: calculate_gldm (cmatrices.c:660-754) -------------------------------------------------- */
/* gldm: float64 [Nvox][Ng][2*Na+1] */
int prad_calculate_gldm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                        const int *angles, int Na, int Ng, int alpha,
                        int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                        double *gldm);
int prad_calculate_gldm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                            const int *angles, int Na, int Ng, int alpha,
                            int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                            double *gldm, void *stream);

/* ---- NGTDM: calculate_ngtdm (cmatrices.c:543-658) ------------------------------------------------ */
/* ngtdm: float64 [Nvox][Ng][3].  Column 1 (sum of |i - mean(neighbours)|) is evaluated as
 * sum_c (sum_p |c*i - s|)/c with exact integer inner sums in segment mode (correctly rounded to a few ulp; the
 * reference's own raster-order sum of Nv rounded terms drifts from that by ~1e-13 .. 1e-12 relative at 10^6
 * voxels -- tests bound the distance to the exact rational value and to the
 * reference's raster-order float64 sum) and in raster order -- bit-identical -- in voxel mode. */
int prad_calculate_ngtdm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                         const int *angles, int Na, int Ng,
                         int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         double *ngtdm);
int prad_calculate_ngtdm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                             const int *angles, int Na, int Ng,
                             int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             double *ngtdm, void *stream);
/* GLDM (cmatrices.c:568-648) and NGTDM (cmatrices.c:650-745) of one segment from ONE pass over the 26 / 8 neighbours
 * (both matrices look at the same neighbourhood; the case pipeline asks for both): device pointers, the bidirectional
 * angle set both classes use, gldm float64 [Ng][2 Na + 1], ngtdm float64 [Ng][3].  Falls back to the two separate calls
 * where the packed-byte kernel does not apply (alpha != 0, rows not a multiple of 4 voxels, Nd > 3).  Deferred mode:
 * enqueue only, as prad_calculate_gldm_dev. */
int prad_calculate_gldm_ngtdm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                                  int Na, int Ng, int alpha, double *gldm, double *ngtdm, void *stream);

/* ---- one large segment over several GPUs: plane-range accumulators of GLDM / NGTDM ------------------
 * (no reference analogue; SURVEY 8e "one exchange step": GLDM / NGTDM histograms are additive over centre
 * voxels.)  acc: DEVICE int64 [Ng][Na+1] for the centre voxels in planes z_lo <= z < z_hi of dim 0 of a 3-D
 * volume, neighbours taken from the whole volume (only planes z_lo-1 .. z_hi are read for distance 1):
 *   family 0, GLDM :  acc[g][k] = voxels of level g+1 with dependence k            (cmatrices.c:737-748)
 *   family 1, NGTDM:  acc[g][0] = voxels of level g+1;  acc[g][c] = sum over those with c valid neighbours
 *                     of |c*level - sum(neighbour levels)|                          (cmatrices.c:637-652)
 * The accumulators of disjoint plane ranges add up (exactly, they are integers) to those of the whole
 * volume; prad_neigh_finalize_dev turns the sum into the matrix prad_calculate_gldm / _ngtdm return
 * (gldm float64 [Ng][2*Na+1], ngtdm float64 [Ng][3]), bit-identical to the single-device call.
 * `alpha` is used by GLDM only.  PRAD_E_UNSUPPORTED when Nd != 3, Ng > 255 or the bins exceed 64 KiB of LDS;
 * PRAD_INDEX_ERROR when a masked level is outside 1..Ng. */
int prad_neigh_accumulate_dev(int family, const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                              const int *angles, int Na, int Ng, int alpha, int z_lo, int z_hi, long long *acc,
                              void *stream);
int prad_neigh_finalize_dev(int family, const long long *acc, int Ng, int Na, double *out, void *stream);

/* ---- GLSZM: calculate_glszm + fill_glszm (cmatrices.c:94-297) ----------------------------------- */
/* Phase 1: labels the zones of every kernel on the device and keeps the (level, size) list in the
 * library's per-thread workspace.  Returns the largest zone size over all Nvox kernels (>= 0), or
 * PRAD_E_* (< 0); *nzones (optional) receives the total number of zones.  `Ns` only sizes scratch in the
 * reference (_cmatrices.c:298-322) but its exhaustion is observable: a kernel with >= 2*Ns zones, or (voxel mode)
 * more than Ns masked voxels, makes the reference fail -- reproduced here as PRAD_E_INDEX (so an empty mask with
 * Ns = 0 raises IndexError exactly like the reference). */
int prad_calculate_glszm(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                         const int *angles, int Na, int Ng, int Ns,
                         int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         long long *nzones);
int prad_calculate_glszm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                             const int *angles, int Na, int Ng, int Ns,
                             int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             long long *nzones, void *stream);
/* Phase 2: histograms the zone list of the preceding phase-1 call into glszm float64
 * [Nvox][Ng][maxRegion] (host pointer for prad_fill_glszm, device pointer for _dev).
 * Returns PRAD_OK, or PRAD_INDEX_ERROR when a zone has level <= 0 or falls outside Ng x maxRegion
 * (cmatrices.c:290-291). */
int prad_fill_glszm(double *glszm, int Nvox, int Ng, int maxRegion);
int prad_fill_glszm_dev(double *glszm, int Nvox, int Ng, int maxRegion, void *stream);
/* Optional: copy the zone list of kernel v to the host in the reference's tempData format
 * (level,size pairs in raster order of each zone's first voxel, terminated by -1; cmatrices.c:255-276).
 * tempData must hold 2*nzones_v+1 ints; returns nzones_v or PRAD_E_*. */
long long prad_glszm_zones(int v, int *tempData, long long capacity_pairs);
/* Optional, segment mode: the matrix with its empty size columns already removed -- what glszm.py:118-131 keeps
 * (`jvector`, `np.delete(P_glszm, emptyZoneSizes, 2)`).  The reference layout [Ng][maxRegion] is almost all
 * zeros once zones are large (maxRegion in the millions for a smooth 256^3 volume, a few thousand distinct sizes).
 * prad_glszm_sizes: the distinct zone sizes of the preceding phase-1 call, ascending, into the HOST array `sizes`
 *   (capacity entries; at most min(maxRegion, sqrt(2 Nvoxels) + 1) are needed); returns their number k or PRAD_E_*.
 * prad_fill_glszm_compact_dev: glszm float64 [Ng][k] (DEVICE pointer), column c counting the zones of size
 *   sizes[c]; PRAD_OK / PRAD_INDEX_ERROR as prad_fill_glszm. */
int prad_glszm_sizes(int *sizes, int capacity);
int prad_fill_glszm_compact_dev(double *glszm, int Ng, int nsizes, void *stream);

/* ---- fused voxel-based GLCM feature maps (no reference analogue at this boundary) ---------------------------
 * For every centre voxel the GLCM of its kernel window is built and reduced to the requested features on the
 * device; the P[Nvox][Ng][Ng][Na] intermediate of the reference (glcm.py:145, base.py:200-245) is never
 * materialised.  Semantics follow glcm.py:149-887 with weightingNorm = None: per-angle normalisation, nanmean over
 * the angles that are non-empty for the voxel.  feature_ids: 0 Autocorrelation, 1 JointAverage, 2 ClusterProminence,
 * 3 ClusterShade, 4 ClusterTendency, 5 Contrast, 6 Correlation, 7 DifferenceAverage, 8 DifferenceEntropy,
 * 9 DifferenceVariance, 10 JointEnergy, 11 JointEntropy, 12 Imc1, 13 Imc2, 14 Idm, 15 Idmn, 16 Id, 17 Idn,
 * 18 InverseVariance, 19 MaximumProbability, 20 SumAverage, 21 SumEntropy, 22 SumSquares (MCC: prad_voxel_glcm_mcc).
 *   out         float64 [nfeat][Nvox]
 *   empty_mask  uint32 [Nvox] (optional): bit a set <=> angle a has no voxel pair in kernel v
 *   any_nonempty uint32 [1] (optional): OR of the non-empty angle bits over all kernels (JointAverage, which the
 *               reference averages with a plain mean, is NaN for kernels whose empty angles are not empty
 *               everywhere -- glcm.py:292; the Python layer applies that rule)
 * Requirements: Nd <= 3, Ng <= 64, Na <= 32, masked levels in [1, Ng]; otherwise PRAD_E_UNSUPPORTED and the
 * caller uses prad_calculate_glcm + host features.  All pointers of the _dev variant are device pointers. */
int prad_voxel_glcm_features(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                             int Na, int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             int symmetric, const int *feature_ids, int nfeat, double *out, uint32_t *empty_mask,
                             uint32_t *any_nonempty);
int prad_voxel_glcm_features_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                 const int *angles, int Na, int Ng, int Nvox, const int *voxels, int kernelRadius,
                                 int force2Ddim, int symmetric, const int *feature_ids, int nfeat, double *out,
                                 uint32_t *empty_mask, uint32_t *any_nonempty, void *stream);

/* MCC (glcm.py:665-707), the one GLCM feature that is an eigenvalue problem: sqrt of the second largest eigenvalue of
 * Q(i,j) = sum_k p(i,k) p(j,k) / (px(i) py(k) + eps), per angle, mean over the non-empty angles (np.nanmean).  One wave
 * per matrix runs a cyclic Jacobi iteration on the symmetric matrix A A^T that is similar to Q, restricted to the grey
 * levels that occur (at most 64 of them; more -> PRAD_E_UNSUPPORTED and the caller's host route).
 *   prad_voxel_glcm_mcc[_dev]  out float64 [Nvox]: per kernel (NaN when no angle has a voxel pair); arguments as for
 *                              prad_voxel_glcm_features
 *   prad_glcm_mcc_dev          glcm: DEVICE float64 raw counts [Ng][Ng][Na] (reference layout); out: HOST float64 [Na],
 *                              NaN for an angle without pairs
 * The reference's "a matrix of a single grey level -> 1" rule (glcm.py:702-703) depends on the grey levels of the whole
 * ROI and stays with the caller. */
int prad_voxel_glcm_mcc(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                        int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, int symmetric, double *out);
int prad_voxel_glcm_mcc_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                            int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, int symmetric,
                            double *out, void *stream);
int prad_glcm_mcc_dev(const double *glcm, int Ng, int Na, int symmetric, double *out, void *stream);

/* Fused voxel-based feature maps of the other four texture classes (same idea, same window rule as above).
 * family: 1 = GLDM (alpha = gldm_a; angles bidirectional), 2 = NGTDM (bidirectional), 3 = GLRLM (unidirectional, mean
 * over the non-empty angles as np.nanmean does), 4 = GLSZM (bidirectional).  feature_ids (HOST) follow the lists
 * VOXEL_*_FEATURES of pyradiomics_amd/cmatrices.py; out is DEVICE float64 [nfeat][Nvox]; image / mask / voxels are
 * DEVICE pointers.  PRAD_E_UNSUPPORTED (Nd > 3, Ng > 255, > 32 angles, > 512 voxels per kernel, levels outside
 * [1, Ng]) means: build the matrices with prad_calculate_* and evaluate the formulas on the host. */
int prad_voxel_texture_features_dev(int family, const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                    const int *angles, int Na, int Ng, int alpha, int Nvox, const int *voxels,
                                    int kernelRadius, int force2Ddim, const int *feature_ids, int nfeat, double *out,
                                    void *stream);

/* ---- segment-mode feature formulas on the device matrices (no reference analogue: numpy in glcm.py:208-887,
 * glrlm.py:174-523, glszm.py:108-434, gldm.py:103-430) ------------------------------------------------------------
 * prad_glcm_features_dev: glcm = DEVICE float64 [Ng][Ng][Na] raw counts as prad_calculate_glcm[_glrlm]_dev leave
 *   them; per angle the matrix is symmetrised (symmetric != 0), normalised, and reduced to the 23 features that are
 *   plain sums (ids = VOXEL_GLCM_FEATURES order; MCC excluded).  out: HOST float64 [Na][23]; empty: HOST int [Na],
 *   1 where the angle holds no pair (its row of `out` is NaN; glcm.py:186-198 drops such angles).
 * prad_zone_matrix_features_dev: P(i, j, a) = P[i*stride_i + j*stride_j + a*stride_a] DEVICE float64 counts with level
 *   value i + 1 and size value jvals[j] (HOST float64 [Nj]: run lengths / zone sizes / dependence counts + 1; NULL: j + 1);
 *   out: HOST float64 [Na][16] in the shared numbering of prad_voxel_texture_features_dev; empty as above. */
int prad_glcm_features_dev(const double *glcm, int Ng, int Na, int symmetric, double *out, int *empty, void *stream);
int prad_zone_matrix_features_dev(const double *P, int Ni, int Nj, int Na, long long stride_i, long long stride_j,
                                  long long stride_a, const double *jvals, double *out, int *empty, void *stream);
/* prad_glszm_features_dev: the GLSZM of a segment (what prad_calculate_glszm_dev + prad_glszm_sizes +
 *   prad_fill_glszm_compact_dev build, cmatrices.c:294-443 / glszm.py:108-131) AND its 16 features, without a host round
 *   trip in between: zones, then the distinct zone sizes are ranked on the device, the compact matrix filled, the
 *   formulas evaluated.  image / mask DEVICE, angles HOST int [Na][Nd] (the bidirectional distance-1 set), Ns = ROI
 *   voxels.  out: float64 [17] -- the 16 features in the shared numbering, then a verdict: 0 = fine, bit 1 = the zone
 *   list would overflow the reference's Ns-sized scratch (cmatrices.c:366-373), other bits = the device-side ranking
 *   declined (levels outside 1..Ng, more than 4096 zones of 8192+ voxels); empty: int [1], 1 = no zone.
 *   Needs the packed-byte tile kernels (Nd <= 3, full 26- / 8-neighbourhood, Ng <= 255): PRAD_E_UNSUPPORTED otherwise,
 *   before anything is launched.  In deferred mode with out / empty inside the result arena: enqueue only, the caller
 *   reads the verdict from out[16] after synchronising; otherwise synchronous, verdict bit 1 -> PRAD_E_INDEX, any other
 *   bit -> PRAD_E_UNSUPPORTED (take the three-call route). */
int prad_glszm_features_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                            int Ng, int Ns, double *out, int *empty, void *stream);
/* NGTDM (ngtdm.py:133-287): P = DEVICE float64 [Ng][3] as prad_calculate_ngtdm_dev leaves it;
 * out: HOST float64 [5] = Coarseness, Contrast, Busyness, Complexity, Strength. */
int prad_ngtdm_features_dev(const double *P, int Ng, double *out, void *stream);

/* ---- on-device discretisation (radiomics/imageoperations.py:67-174; device pointers only) ----------------------
 * dtype: 0 = float32, 1 = float64, 2 = int32, 3 = int16 image.
 * prad_roi_minmax_dev: minmax[0..1] (HOST doubles) = min / max of image over mask != 0; PRAD_E_ARG if the ROI is empty.
 * prad_digitize_dev:   levels[i] = number of edges <= image[i] (np.digitize) where mask != 0, else 0;
 *                      `edges` is a HOST array of nedges ascending float64 values (getBinEdges output);
 *                      *max_level (HOST int) receives the largest level written (= Ng of base.py:121-124).
 * prad_level_counts_dev: counts[g] (HOST int64, Ng + 1 entries) = number of ROI voxels with level g for g in 1..Ng
 *                      (which levels are present = `grayLevels` of base.py:120-122, their sum = Ns of glszm.py:84);
 *                      counts[0] = ROI voxels whose level is outside 1..Ng. */
int prad_roi_minmax_dev(const void *image, int dtype, const uint8_t *mask, long long n, double *minmax, void *stream);
int prad_digitize_dev(const void *image, int dtype, const uint8_t *mask, long long n, const double *edges, int nedges,
                      int32_t *levels, int *max_level, void *stream);
int prad_level_counts_dev(const int32_t *levels, const uint8_t *mask, long long n, int Ng, long long *counts,
                          void *stream);
/* prad_digitize_counts_dev: prad_digitize_dev and the level census in ONE pass over the image (base.py:119-125 needs
 *                      both for every derived image): counts (HOST int64, nedges + 1 entries, may be NULL) receives the
 *                      number of ROI voxels per level 0..nedges.  Any number of edges (beyond 7 680 the edge list is
 *                      searched in global memory instead of LDS). */
int prad_digitize_counts_dev(const void *image, int dtype, const uint8_t *mask, long long n, const double *edges,
                             int nedges, int32_t *levels, int *max_level, long long *counts, void *stream);
/* binCount discretisation with ONE host synchronisation: ROI min / max, the np.histogram edges built on the device
 * (np.linspace's arithmetic: i * step + min with two roundings, last edge = max, then + 1 as in imageoperations.py:122-126;
 * in float32 for a float32 image, as numpy does it, in float64 otherwise), levels, largest level and the level census in
 * one queue.  dtype as for prad_digitize_dev.  minmax: HOST double [2]; edges:
 * HOST double [binCount + 1] or NULL (what the device used: bit-identical to getBinEdges on (min, max));
 * counts: HOST int64 [binCount + 2] as prad_digitize_counts_dev, or NULL.  PRAD_E_UNSUPPORTED for a constant or
 * non-finite ROI (np.histogram widens the range then): the two-call route with host-built edges serves those. */
int prad_bincount_dev(const void *image, int dtype, const uint8_t *mask, long long n, int binCount, int32_t *levels,
                      double *minmax, double *edges, int *max_level, long long *counts, void *stream);
/* prad_bincount_dev in two halves, for callers that have other host work between "queued" and "needed" (the case pipeline
 * bins derived image i + 1 while the host still collects image i: imageoperations.py:67-174 + base.py:119-125 are one
 * synchronous step per feature class in the reference).  prad_bincount_enqueue_dev queues the same kernels and the copy of
 * their 8 x (2 binCount + 7) result bytes into a pinned block and returns a ticket (up to four in flight per host thread);
 * prad_bincount_wait waits for THAT work only (an event behind the copy) and fills the host outputs of prad_bincount_dev,
 * with its return codes.  A ticket is waited for exactly once; `levels` must stay allocated until then. */
int prad_bincount_enqueue_dev(const void *image, int dtype, const uint8_t *mask, long long n, int binCount, int32_t *levels,
                              int *ticket, void *stream);
int prad_bincount_wait(int ticket, double *minmax, double *edges, int *max_level, long long *counts);

/* ---- first-order statistics of the ROI intensities (radiomics/firstorder.py:33-474; device pointers) -----------
 * Segment mode.  The reference computes these with numpy on image[mask] (firstorder.py:96-101); here the ROI is
 * compacted, sorted and reduced on the device and `out` (HOST, PRAD_FO_COUNT doubles) receives the statistics every
 * feature of the class derives from:
 *   Np; Energy = sum (x + voxelArrayShift)^2 (:151); Minimum / Maximum (:207,:244); the 10 / 25 / 75 / 90-th
 *   percentiles and the median with numpy's linear interpolation (:218-231,:268,:282); Mean (:256); mean absolute
 *   deviation (:308); robust mean absolute deviation over p10 <= x <= p90 (:323-342); central moments m2, m3, m4
 *   (:136-145, Variance / Skewness / Kurtosis :381-446).
 * dtype as for prad_digitize_dev.  Entropy / Uniformity come from prad_level_counts_dev on the discretised image. */
enum { PRAD_FO_NP = 0, PRAD_FO_ENERGY, PRAD_FO_MINIMUM, PRAD_FO_P10, PRAD_FO_P25, PRAD_FO_MEDIAN, PRAD_FO_P75, PRAD_FO_P90,
       PRAD_FO_MAXIMUM, PRAD_FO_MEAN, PRAD_FO_MAD, PRAD_FO_RMAD, PRAD_FO_M2, PRAD_FO_M3, PRAD_FO_M4, PRAD_FO_COUNT };
int prad_firstorder_dev(const void *image, int dtype, const uint8_t *mask, long long n, double voxelArrayShift,
                        double *out, void *stream);
/* The same statistics without a host round trip between the passes (prad_firstorder_dev has five): what the host does
 * in between -- adding up block partials, placing the quantiles, finding the histogram bins that hold their ranks,
 * interpolating -- runs in single-workgroup kernels on a device record, the same operations in the same order (the same
 * bits).  float32 / float64 images with roi_count >= 2^20 ROI voxels (the caller knows the count from the level census);
 * PRAD_E_UNSUPPORTED otherwise, before anything is launched.  out: 16 doubles -- the PRAD_FO_COUNT statistics, then a
 * verdict (0 = fine; 1: the ROI holds a different number of voxels, 2: constant or non-finite ROI, 8: the selected
 * histogram bins hold more than the gather capacity: half of the ROI, at least 2^18 voxels).  In deferred mode with `out` inside the result arena: enqueue only;
 * otherwise synchronous, a non-zero verdict returns PRAD_E_UNSUPPORTED (call prad_firstorder_dev). */
int prad_firstorder_queue_dev(const void *image, int dtype, const uint8_t *mask, long long n, long long roi_count,
                              double voxelArrayShift, double *out, void *stream);
/* Voxel mode (firstorder.py:37-118,104-118): for each of the Nvox centres (`voxels` DEVICE int32 [Nd][Nvox]) the
 * window centre + {offsets of infinity-norm <= kernelRadius} -- per dimension limited to |offset| < bbsize[d] (HOST,
 * the `boundingBoxSize` of firstorder.py:45-58; NULL = no limit) and 0 in the force2D dimension -- is reduced over
 * its voxels with mask != 0 (the reference's NaN padding / NaN outside the ROI).  levels (discretised image, may
 * be NULL) feeds Entropy / Uniformity.  feature_ids (HOST) index the feature list in the order of
 * pyradiomics_amd.firstorder.FEATURES; out is DEVICE float64 [nfeat][Nvox]. */
int prad_voxel_firstorder_dev(const void *image, int dtype, const uint8_t *mask, const int32_t *levels, const int *size,
                              int Nd, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, const int *bbsize,
                              double voxelArrayShift, double voxelVolume, const int *feature_ids, int nfeat, double *out,
                              void *stream);

/* ---- resampling in front of the path (radiomics/imageoperations.py:448-612 on SimpleITK's ResampleImageFilter) ------
 * Output voxel o along (numpy) axis d samples the input at the continuous index start[d] + o * step[d]; the output
 * grid shares the input's axes (the reference derives start / step / newsize from the ROI bounding box, padDistance
 * and resampledPixelSpacing, imageoperations.py:548-578).  interpolator: 0 nearest neighbour (round half up), 1 linear,
 * 3 cubic B-spline exactly as ITK evaluates it (recursive prefilter with mirror boundaries, mirrored 4^Nd support);
 * samples outside the buffer ([-0.5, N - 0.5) per axis) become 0; integer pixel types are clamped and truncated like
 * ResampleImageFilter::CastPixelWithBoundsChecking.  image / out: DEVICE pointers of the same dtype (codes as for
 * prad_digitize_dev); size / start / step / newsize: HOST arrays of Nd (<= 3) entries. */
int prad_resample_dev(const void *image, int dtype, const int *size, int Nd, const double *start, const double *step,
                      const int *newsize, int interpolator, void *out, void *stream);

/* ---- label census: every label of a label map in one pass (no reference analogue: the reference extracts one label per
 * execute() call and finds its ROI with sitk.LabelStatisticsImageFilter, imageoperations.py:407-445) ------------------
 * mask: integer label map [size[0]]..[size[Nd-1]], Nd = 2 or 3, C-contiguous; dtype: 2 = int32, 3 = int16 (the codes of
 * prad_digitize_dev) or 4 = uint8.  table: int64 [max_label + 1][1 + 2 Nd], row v = voxel count of label v, then lo[Nd] and
 * hi[Nd], its inclusive index bounds in array (z, y, x) order.  Row 0 (background) is zero; values below 1 or above
 * max_label are ignored; a label that does not occur has count 0, lo[d] = size[d], hi[d] = -1.  0 <= max_label <= 65535
 * (PRAD_E_ARG beyond: the caller looks at such a map label by label).  The table need not be initialised.
 * One pass over the map: a wave that finds one value in all of its lanes adds a whole row piece to a run it keeps in
 * registers; tables of up to 12288 words are kept per workgroup in LDS and merged at its end (prad_last_variant:
 * "census-lds"), larger ones are updated in global memory ("census-global").  Integer atomics: exact, order-independent.
 * prad_label_census_dev: device pointers, synchronises `stream`; prad_label_census: host pointers, staged.
 * prad_mask_max_dev: *max_value (HOST) = largest element of the n elements of `mask` (DEVICE), to size the table. */
int prad_label_census_dev(const void *mask, int dtype, const int *size, int Nd, int max_label, long long *table, void *stream);
int prad_label_census(const void *mask, int dtype, const int *size, int Nd, int max_label, long long *table);
int prad_mask_max_dev(const void *mask, int dtype, long long n, long long *max_value, void *stream);

/* ---- many small ROIs, one launch (no reference analogue: the reference builds one segment per call) --------------------
 * B independent ROIs stored back to back: ROI b is the int32 level box [size[b][0]][size[b][1]][size[b][2]] (z, y, x,
 * C-contiguous) that starts at ELEMENT off[b] of `levels`, with its uint8 mask at the same element of `mask`.  One
 * workgroup per (ROI, angle group) packs the box into LDS and builds its matrices there (csrc/kernels_batch.h); every
 * matrix equals what the single segment-mode call returns for that box:
 *   PRAD_BATCH_GLCM   prad_calculate_glcm_dev   [Ng][Ng][Na]        Na = prad_get_angle_count(size, distances, unidirectional);
 *                                                                   not symmetrised, as there
 *   PRAD_BATCH_GLRLM  prad_calculate_glrlm_dev  [Ng][Nr][Na1]       Nr = max(size[b]); Na1 = the distance-1 count: the
 *                                                                   reference's GLRLM ignores `distances` (_cmatrices.c:432-581)
 *   PRAD_BATCH_GLDM   prad_calculate_gldm_dev   [Ng][2 Nb + 1]      Nb = 2 Na, the bidirectional count that call is given
 *   PRAD_BATCH_NGTDM  prad_calculate_ngtdm_dev  [Ng][3]             (float column: the same sum as the single call, bit for bit)
 * Each family is ONE flat float64 buffer, ROI after ROI; the call writes every element (no pre-zeroing).
 * prad_batch_plan (host only, needs no device): out_offsets int64 [4][B + 1], row f (0 GLCM, 1 GLRLM, 2 GLDM, 3 NGTDM) =
 *   first double of every ROI in that family's buffer and, at [B], the buffer's length (all zero for a family that is not in
 *   `families`); Na int [2][B] = Na, then Na1.  Returns PRAD_OK, or PRAD_E_UNSUPPORTED -- outputs filled all the same -- when
 *   prad_calculate_batch_dev would decline the batch.
 * prad_calculate_batch_dev: levels / mask / outputs / status are DEVICE pointers, sizes ([B][3]) / off / distances HOST.
 *   status int [B]: PRAD_OK, or PRAD_INDEX_ERROR for a ROI with a masked level outside [1, Ng] (the reference's IndexError;
 *   its matrices are then those of an empty mask, the other ROIs are not affected).  An empty mask and a 1 x 1 x 1 box
 *   (Na = 0: empty GLCM / GLRLM) are legal.  Covered: 1 <= Ng <= 64, boxes of at most prad_batch_max_vox() voxels, at most
 *   127 angles per ROI; anything else returns PRAD_E_UNSUPPORTED for the whole batch before a launch (loop the single calls).
 *   Enqueues one copy and one launch on `stream` and synchronises it; kernel family "batch" (prad_last_kernel_ms);
 *   prad_last_path: "batch".  GLSZM has entry points of its own (below): the shape of its output depends on the data. */
#define PRAD_BATCH_GLCM 1
#define PRAD_BATCH_GLRLM 2
#define PRAD_BATCH_GLDM 4
#define PRAD_BATCH_NGTDM 8
#define PRAD_BATCH_ALL 15
int prad_batch_max_vox(void);
int prad_batch_plan(const int *sizes, int B, int Ng, int families, const int *distances, int Ndist, long long *out_offsets,
                    int *Na);
int prad_calculate_batch_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, int Ng,
                             int families, const int *distances, int Ndist, int alpha, double *glcm, double *glrlm,
                             double *gldm, double *ngtdm, int *status, void *stream);
/* force2D on the batched route.  force2Ddim: -1 none -- the two functions above are these with -1 --, or 0 / 1 / 2, the axis (z,
 * y, x) that no angle may leave: the last argument of prad_get_angle_count / prad_build_angles, from which the counts and the
 * angle tables of every ROI come, as they do for the single calls.  Everything else is as above: the same layouts with the
 * forced Na / Na1, the same domain, the same synchronisation.  A ROI whose angles all vanish under the forced dimension (a
 * 5 x 1 x 1 box with dimension 0; the 1 x 1 x 1 box with any) is legal: Na = Na1 = 0, its GLCM and GLRLM are empty, its GLDM
 * [Ng][1] counts the masked voxels per level and its NGTDM is (count, 0, level): the matrices of voxels without neighbours,
 * what the reference's cmatrices.c computes from an empty angle table.  prad_last_path "batch"; prad_last_variant "batch-lds"
 * for -1, "batch-lds-f2d" otherwise (the kernel is the same one: it consumes whatever table it is given). */
int prad_batch_plan_f2d(const int *sizes, int B, int Ng, int families, const int *distances, int Ndist, int force2Ddim,
                        long long *out_offsets, int *Na);
int prad_calculate_batch_f2d_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                 int Ng, int families, const int *distances, int Ndist, int alpha, int force2Ddim, double *glcm,
                                 double *glrlm, double *gldm, double *ngtdm, int *status, void *stream);
/* A grey-level count PER ROI.  The *_ng entry points of the batched texture route take `const int *Ng`, a HOST vector [B], where
 * the calls above and below take `int Ng`; ROI b then has Ng[b] levels: its matrices are [Ng[b]][...] in every layout, its
 * masked levels must lie in [1, Ng[b]] (status PRAD_INDEX_ERROR otherwise, whatever the counts of the other ROIs) and a plan's
 * offsets advance by its own shapes.  This is what a fixed bin width gives a table of lesions.  The scalar entry points are these
 * with the same count for every ROI -- one implementation --, so everything said of them holds: layouts, status, domain,
 * synchronisation, kernel family, prad_last_path / prad_last_variant.  Domain: any Ng[b] < 1 is PRAD_E_ARG; any Ng[b] > 64 is
 * PRAD_E_UNSUPPORTED for the whole batch before anything is launched or written (a plan fills its outputs all the same): the
 * caller partitions the batch.  A NULL vector with B > 0 is PRAD_E_ARG.  The LDS tables of the matrix launch are sized by the
 * most any ROI asks for with its own count, within the budget, and never below the smallest whole table of every ROI. */
int prad_batch_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *distances, int Ndist, int force2Ddim,
                       long long *out_offsets, int *Na);
int prad_calculate_batch_ng_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                const int *Ng, int families, const int *distances, int Ndist, int alpha, int force2Ddim,
                                double *glcm, double *glrlm, double *gldm, double *ngtdm, int *status, void *stream);

/* ---- GLSZM of many small ROIs (csrc/kernels_batch_glszm.h) -------------------------------------------------------------
 * The same batch layout (levels / mask DEVICE, sizes [B][3] / off HOST).  One workgroup per ROI packs the box into LDS and
 * labels its zones there -- the full 26-neighbourhood at distance 1 inside the box, which is the angle set the single call
 * is given for a 3-D segment (an axis of length 1 has no neighbours along it) -- then a second launch histograms the zone
 * lists.  Between the two the caller reads `summary` back and lays the matrices out: their shapes depend on the data.
 * prad_batch_glszm_dev: all outputs are DEVICE pointers.
 *   zones   int32: the zone list of ROI b starts at int 2 * off[b] and may use 2 * nvox_b ints (a ROI has at most nvox
 *           zones): (level, size) pairs in the reference's tempData order, raster order of each zone's first voxel
 *           (cmatrices.c:255-276), without the closing -1.  The ints of the region beyond the 2 * summary[b][0] of the pairs
 *           hold scratch values.
 *   summary int32 [B][3]: number of zones, largest zone size (0 if none), number of distinct zone sizes
 *   status  int32 [B]: PRAD_OK, or PRAD_INDEX_ERROR for a ROI with a masked level outside [1, Ng]; that ROI is void (no
 *           zones, summary 0, 0, 0), the others are not affected.  An empty mask gives no zones and PRAD_OK (the single
 *           call's answer for Ns >= 1).
 *   Covered: 1 <= Ng <= 64 and boxes of at most prad_batch_glszm_max_vox() = 54528 voxels (37^3 fits); anything else returns
 *   PRAD_E_UNSUPPORTED for the whole batch after the arguments are checked and before anything is launched or written.
 * prad_batch_glszm_fill_dev: zones / out / sizes_out DEVICE, summary_host (the summary read back) / off / the offsets HOST.
 *   compact == 0: out + out_offsets[b] is float64 [Ng][max(summary[b][1], 1)], the layout of prad_fill_glszm_dev;
 *   compact != 0: float64 [Ng][max(summary[b][2], 1)], column c counting the zones of the c-th distinct size, and
 *   sizes_out + sizes_offsets[b] int32 [summary[b][2]] ascending: prad_glszm_sizes + prad_fill_glszm_compact_dev.
 *   Every element of a ROI's slice is written, zeros included.  A pair that does not fit the summary is skipped.
 * Both enqueue one copy and one launch on `stream` and synchronise it; kernel family "batch_glszm"; prad_last_path "batch",
 * prad_last_variant "batch-glszm-lds". */
int prad_batch_glszm_max_vox(void);
int prad_batch_glszm_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, int Ng,
                         int *zones, int *summary, int *status, void *stream);
int prad_batch_glszm_fill_dev(const int *zones, const int *summary_host, const long long *off, int B, int Ng, int compact,
                              double *out, const long long *out_offsets, int *sizes_out, const long long *sizes_offsets,
                              void *stream);
/* prad_batch_glszm_f2d_dev: prad_batch_glszm_dev (which is this call with force2Ddim = -1) with the neighbourhood of force2D:
 *   force2Ddim 0 / 1 / 2 joins a voxel to its up to 8 neighbours in the plane of the two OTHER axes (z, y, x) -- the angle
 *   set the single call is given with that forced dimension --, so zones never cross a plane.  The neighbourhood is a
 *   compile-time variant of the labelling kernel; outputs, order of the zone list, domain (the LDS budget does not depend on
 *   the neighbourhood: prad_batch_glszm_max_vox()) and synchronisation are unchanged, and prad_batch_glszm_fill_dev serves
 *   all variants.  prad_last_path "batch"; prad_last_variant "batch-glszm-lds" for -1, "batch-glszm-lds-f2d0" / "-f2d1" /
 *   "-f2d2" otherwise.  A force2Ddim outside [-1, 2] is PRAD_E_ARG. */
int prad_batch_glszm_f2d_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, int Ng,
                             int force2Ddim, int *zones, int *summary, int *status, void *stream);
/* The same two calls with a grey-level count per ROI (HOST int [B], see prad_batch_plan_ng): the labelling launch checks ROI b's
 * levels against Ng[b]; the fill writes float64 [Ng[b]][cols_b] at out + out_offsets[b]. */
int prad_batch_glszm_ng_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                            const int *Ng, int force2Ddim, int *zones, int *summary, int *status, void *stream);
int prad_batch_glszm_fill_ng_dev(const int *zones, const int *summary_host, const long long *off, int B, const int *Ng,
                                 int compact, double *out, const long long *out_offsets, int *sizes_out,
                                 const long long *sizes_offsets, void *stream);

/* ---- feature formulas of many small ROIs (csrc/kernels_batch_features.h) -------------------------------------------------
 * The formulas of prad_glcm_features_dev, prad_glcm_mcc_dev, prad_zone_matrix_features_dev and prad_ngtdm_features_dev on the
 * flat buffers of the two batched matrix calls above: one launch for every matrix of the batch, a second one for MCC.  A
 * workgroup evaluates one matrix with the device function, the thread count and the order of additions of the single call, so
 * every value equals the single call's bit for bit.  ROI b produces, in one flat float64 output,
 *   PRAD_BATCH_GLCM   Na_b rows of 24: the 23 sum features in the order of prad_glcm_features_dev, then MCC (NaN for an angle
 *                     without pairs, and everywhere when want_mcc == 0)
 *   PRAD_BATCH_GLRLM  Na1_b rows of 16 (size values 1 .. max(size[b]))
 *   PRAD_BATCH_GLDM   one row of 16 (size values 1 .. 2 Nb + 1)
 *   PRAD_BATCH_NGTDM  one row of 5
 *   PRAD_BATCH_GLSZM  one row of 16; glszm_cols[b] = columns of the ROI's matrix [Ng][glszm_cols[b]], i.e. max(summary[b][2], 1)
 *                     compact and max(summary[b][1], 1) dense.  glszm_cols[b] <= 0: the ROI's GLSZM is not in the buffer (it
 *                     was outside the domain of prad_batch_glszm_dev); its row is laid out but not written.
 * and one int32 `empty` flag per row (1: the matrix is all zero and the row is NaN; NGTDM: no level occurs, the row is what
 * prad_ngtdm_features_dev gives).  Na is the int [2][B] of prad_batch_plan.
 * prad_batch_features_plan (host only, needs no device).  Deviations from a plain row table, because rows differ in width:
 *   out_offsets int64 [2][5][B + 1]: [0][f][b] = first DOUBLE of ROI b's rows of family f (0 GLCM .. 3 NGTDM, 4 GLSZM) in `out`,
 *   [1][f][b] = its first ROW, i.e. index into `empty`; families follow one another, [.][f][B] = end of family f (a family
 *   that is not asked for takes no space); nrec int64 [3] = records (workgroups) of the first launch, GLCM angles (workgroups
 *   of the MCC launch), doubles of scratch.  Returns PRAD_OK, or PRAD_E_UNSUPPORTED -- outputs filled all the same -- when
 *   prad_batch_features_dev would decline: covered is 1 <= Ng <= 64.
 * prad_batch_features_dev: sizes / Na / glszm_cols / offsets / glszm_offsets / glszm_sizes_offsets HOST; the matrices,
 *   glszm_sizes, out and empty DEVICE.  offsets int64 [4][B + 1] as prad_batch_plan writes them (only [f][b], b < B, is read:
 *   the first double of ROI b's matrix, which has the shape prad_calculate_batch_dev gives it); glszm_offsets int64 [B] likewise
 *   for the GLSZM buffer.  glszm_sizes: the int32 sizes_out of prad_batch_glszm_fill_dev with glszm_sizes_offsets [B] (an entry
 *   < 0: size value j + 1 for that ROI); NULL: dense matrices, size value j + 1.  The size values are widened to double in the
 *   kernel (exact).  Buffers of families that are not asked for may be NULL.  Anything outside the domain returns
 *   PRAD_E_UNSUPPORTED before a launch and writes nothing.  Enqueues one copy and one launch (two with want_mcc) on `stream`
 *   and synchronises it; kernel family "batch_features"; prad_last_path "batch", prad_last_variant "batch-features". */
#define PRAD_BATCH_GLSZM 16
#define PRAD_BATCH_FEATURES_ALL 31
int prad_batch_features_plan(const int *sizes, int B, int Ng, int families, const int *Na, const int *glszm_cols,
                             long long *out_offsets, long long *nrec);
int prad_batch_features_dev(const int *sizes, int B, int Ng, int families, const int *Na, const int *glszm_cols,
                            const double *glcm, const double *glrlm, const double *gldm, const double *ngtdm,
                            const long long *offsets, const double *glszm, const long long *glszm_offsets,
                            const int *glszm_sizes, const long long *glszm_sizes_offsets, int symmetric, int want_mcc,
                            double *out, int *empty, void *stream);
/* The same two calls with a grey-level count per ROI (HOST int [B], see prad_batch_plan_ng): the matrices of ROI b have Ng[b]
 * rows (GLCM: and columns), as prad_calculate_batch_ng_dev and prad_batch_glszm_fill_ng_dev write them.  The row layout of `out`
 * does not depend on the counts; the scratch in nrec[2] does. */
int prad_batch_features_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *Na, const int *glszm_cols,
                                long long *out_offsets, long long *nrec);
int prad_batch_features_ng_dev(const int *sizes, int B, const int *Ng, int families, const int *Na, const int *glszm_cols,
                               const double *glcm, const double *glrlm, const double *gldm, const double *ngtdm,
                               const long long *offsets, const double *glszm, const long long *glszm_offsets,
                               const int *glszm_sizes, const long long *glszm_sizes_offsets, int symmetric, int want_mcc,
                               double *out, int *empty, void *stream);

/* ---- weighted angle merge of many small ROIs: weightingNorm (csrc/kernels_batch_merge.h) --------------------------------------
 * One launch for the whole batch turns the per-angle GLCM and GLRLM buffers of prad_calculate_batch[_f2d]_dev into ONE matrix
 * per ROI, what the feature classes form with weightingNorm set:
 *   PRAD_BATCH_GLCM   glcm_w  float64 [Ng][Ng][1]       glcm_w[i][j]  = sum_a w_a * (P[i][j][a] + (symmetric ? P[j][i][a] : 0))
 *   PRAD_BATCH_GLRLM  glrlm_w float64 [Ng][Nr][1]       glrlm_w[i][r] = sum_a w_a * R[i][r][a],   Nr = max(size[b])
 * ROI after ROI in flat buffers.  The sum runs over a ascending from 0.0, every term a rounded product followed by a rounded add
 * (no FMA contraction), so the result depends on the inputs alone and equals the host loop `acc = acc + P[..., a] * w[a]` bit
 * for bit.  Work is divided by output cells (records of up to 1024 cells of one matrix), every element is written, a ROI with
 * no angle of a family or with status != PRAD_OK gets zeros.  prad_batch_features_dev then takes the merged buffers with Na =
 * Na1 = 1 for every ROI and symmetric = 0 (the merge has symmetrised); MCC is evaluated on the merged matrix.
 * prad_batch_merge_plan (host only, needs no device): Na is the int [2][B] of prad_batch_plan[_f2d]; out_offsets int64
 *   [3][B + 1]: row 0 / 1 = first double of ROI b in glcm_w / glrlm_w (all zero for a family not in `families`), row 2 = first
 *   weight of ROI b in `weights`; [.][B] = the lengths.  The weights of ROI b are Na[0][b] doubles for its GLCM angles followed
 *   by Na[1][b] doubles for its GLRLM angles, each in the order of the ROI's rows of prad_build_angles (both always present,
 *   whatever `families`).
 * prad_batch_merge_angles_dev: sizes / Na / offsets / weights HOST; glcm / glrlm / status / glcm_w / glrlm_w DEVICE.  offsets
 *   int64 [4][B + 1] as prad_batch_plan[_f2d] writes them (rows 0 and 1 are read); status: the int [B] of the matrix call, or
 *   NULL (every ROI counts).  families: a non-empty subset of PRAD_BATCH_GLCM | PRAD_BATCH_GLRLM, else PRAD_E_ARG.  Covered:
 *   every valid argument with fewer than 2^31 cells per matrix.  Enqueues one copy (records and weights) and one launch on
 *   `stream` and synchronises it; kernel family "batch_merge"; prad_last_path "batch", prad_last_variant "batch-merge". */
int prad_batch_merge_plan(const int *sizes, int B, int Ng, int families, const int *Na, long long *out_offsets);
int prad_batch_merge_angles_dev(const int *sizes, int B, int Ng, int families, const int *Na, const double *glcm,
                                const double *glrlm, const long long *offsets, const double *weights, const int *status,
                                int symmetric, double *glcm_w, double *glrlm_w, void *stream);
/* The same two calls with a grey-level count per ROI (HOST int [B], see prad_batch_plan_ng): glcm_w of ROI b is [Ng[b]][Ng[b]][1],
 * glrlm_w [Ng[b]][Nr][1].  The merge has no upper bound on the counts. */
int prad_batch_merge_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *Na, long long *out_offsets);
int prad_batch_merge_angles_ng_dev(const int *sizes, int B, const int *Ng, int families, const int *Na, const double *glcm,
                                   const double *glrlm, const long long *offsets, const double *weights, const int *status,
                                   int symmetric, double *glcm_w, double *glrlm_w, void *stream);

/* ---- first-order statistics and discretisation of many small ROIs (csrc/kernels_batch_firstorder.h) --------------------
 * The front end of the batched route: raw intensity boxes in, the statistics of prad_firstorder_dev and the levels and level
 * counts of prad_digitize_counts_dev out, one launch each for the whole batch, one workgroup per ROI.  The batch layout is that
 * of the calls above, in the image's own dtype (codes of prad_digitize_dev: 0 float32, 1 float64, 2 int32, 3 int16): ROI b is
 * the box [size[b][0]][size[b][1]][size[b][2]] at ELEMENT off[b] of `image` (DEVICE), its uint8 mask at the same element of
 * `mask` (DEVICE); sizes ([B][3]) and off are HOST arrays.
 * prad_batch_firstorder_max_roi(dtype): the key capacity, i.e. the most ROI voxels (mask != 0) a workgroup sorts in LDS: 32768
 *   for the 4-byte keys of float32 / int32 / int16, 16384 for float64 (128 KiB of keys); PRAD_E_ARG for another dtype.
 * prad_batch_firstorder_plan (host only, needs no device): *lds_bytes = the dynamic LDS the launch asks for -- 64 bytes + one
 *   key per slot, slots = the next power of two >= min(largest box, capacity), so a batch of 16^3 boxes runs many workgroups
 *   per CU; inside int [B] = 1 where the box itself holds no more voxels than the capacity (the ROI is then certainly served),
 *   0 where that depends on the mask.  PRAD_E_ARG for a bad dtype, B < 1 or a size < 1; PRAD_E_UNSUPPORTED -- outputs filled all
 *   the same -- when prad_batch_firstorder_dev would decline: a box above 2^31 - 1 voxels.
 * prad_batch_firstorder_dev: table DEVICE float64 [B][16]: the PRAD_FO_COUNT statistics in the enum's order, then a verdict:
 *   0 fine; 1 empty ROI (prad_firstorder_dev's PRAD_E_ARG); 2 a non-finite ROI value; 8 more ROI voxels than the capacity.
 *   The 15 statistics are NaN unless the verdict is 0; verdicts 2 and 8: give that ROI to prad_firstorder_dev.  Minimum, Maximum,
 *   the percentiles and Median are those of prad_firstorder_dev bit for bit; the sums run over the ROI's SORTED values (thread t
 *   of 256 adds elements t, t + 256, ..., then 6 shuffle steps and 3 additions), Mean is one float64 division, MAD / m2 / m3 / m4
 *   are taken about that Mean and rMAD about the float64 mean of the band P10 <= x <= P90, so a ROI's row depends on its values
 *   alone -- not on the other ROIs, its place in the batch or the timing of the launch.  Boxes of up to 2^31 - 1 voxels are legal.
 * prad_batch_digitize_dev: edges DEVICE float64, the ascending edges of ROI b (np.digitize's `bins`, built on the host by
 *   getBinEdges from the ROI's Minimum / Maximum) at edge_off[b] .. edge_off[b + 1] - 1 (edge_off HOST int64 [B + 1]).  levels
 *   DEVICE int32, the batch layout: levels[i] = number of edges <= (double)image[i] where mask != 0 (the comparisons of
 *   prad_digitize_dev), 0 elsewhere; every element of every served box is written.  counts DEVICE int64: the ROI voxels per level
 *   0 .. nedges of ROI b at count_off[b] (HOST int64 [B]); top DEVICE int [B]: the largest level.  count_off[b] < 0: the ROI is not
 *   served (nothing of it is written: the caller bins it with prad_digitize_counts_dev).  A ROI without edges gets level 0
 *   throughout.  Covered: at most prad_batch_digitize_max_edges() = 8192 edges per served ROI (edges and counters share the LDS:
 *   12 bytes per edge, 96 KiB at the cap); beyond it PRAD_E_UNSUPPORTED before anything is launched or written.
 * Both enqueue one copy and one launch on `stream` and synchronise it; kernel family "batch_firstorder" (prad_last_kernel_ms);
 * prad_last_path "batch", prad_last_variant "batch-firstorder-lds" / "batch-digitize-lds". */
int prad_batch_firstorder_max_roi(int dtype);
int prad_batch_firstorder_plan(const int *sizes, int B, int dtype, long long *lds_bytes, int *inside);
int prad_batch_firstorder_dev(const void *image, int dtype, const uint8_t *mask, const int *sizes, const long long *off, int B,
                              double voxelArrayShift, double *table, void *stream);
int prad_batch_digitize_max_edges(void);
int prad_batch_digitize_dev(const void *image, int dtype, const uint8_t *mask, const int *sizes, const long long *off, int B,
                            const double *edges, const long long *edge_off, int32_t *levels, long long *counts,
                            const long long *count_off, int *top, void *stream);

/* ---- the boxes of many labels of one label map, packed for the calls above (csrc/kernels_batch_gather.h) -----------------
 * prad_batch_gather_dev copies B boxes out of a 3-D volume into the batch layout in ONE launch: ROI b is the box of extent
 * box[b] ([B][3], z y x) whose first voxel is lo[b] ([B][3]); its voxels go, z-major, to elements offsets[b] .. of out_image
 * (the image's own dtype: codes 0 float32, 1 float64, 2 int32, 3 int16; values are moved bit for bit) and of out_mask (uint8:
 * labelmap == labels[b], so voxels of other labels inside the box are outside the ROI; label codes of prad_label_census_dev:
 * 2 int32, 3 int16, 4 uint8).  image / out_image NULL: masks only; labelmap / out_mask NULL: images only.  image, labelmap and
 * the outputs are DEVICE buffers; size ([3]), labels, lo, box and offsets are HOST arrays.
 * Work is divided by output elements -- workgroups take 1024 consecutive elements of the packed output and find their ROIs in a
 * device table -- so one large box among hundreds of small ones does not serialise on one workgroup.  Volumes and batches
 * above 2^31 elements are legal: every index is 64-bit.  The device table is kept between calls: a call whose tables equal
 * those of the previous call on this thread, device and stream (the masks, then every derived image of one label map) uploads
 * nothing.  One launch on `stream`, no host synchronisation; kernel family "batch_gather", prad_last_variant "batch-gather".
 * PRAD_E_ARG, before anything is launched: a box that leaves the volume, an extent < 1, offsets[b] before the end of ROI b - 1,
 * an input without its output, a dtype code outside the lists. */
int prad_batch_gather_dev(const void *image, int image_dtype, const void *labelmap, int label_dtype, const int *size, int B,
                          const int *labels, const int *lo, const int *box, const long long *offsets, void *out_image,
                          unsigned char *out_mask, void *stream);

/* ---- the wavelet sub-bands of many small boxes (csrc/kernels_batch_swt.h) ----------------------------------------------
 * prad_batch_swt_dev: the level-1, undecimated, periodised 3-D transform of B boxes in ONE launch -- per box what
 * getWaveletImage computes on it: one wrapped sample appended to every odd axis (imageoperations.py:914-919), pywt.swtn over
 * axes (2, 1, 0), the pad cropped again -- with the pad folded into the kernel's index arithmetic.  `in` (DEVICE) holds the boxes
 * in the batch layout of prad_batch_firstorder_dev, in the image's own dtype (0 float32, 1 float64, 2 int32, 3 int16; widened
 * to float64 when staged: exact); sizes ([B][3], z y x), off (element offsets, ascending, boxes not overlapping) and the flen
 * taps of dec_lo / dec_hi are HOST arrays.  out DEVICE float64 [8][band_stride], band_stride >= off[B - 1] + its voxels: band k
 * of ROI b lies at out + k * band_stride + off[b] in the box's own shape, k = (bx * 2 + by) * 2 + bz as prad_swt_level1_dev
 * numbers the bands for axes (2, 1, 0) -- every out[k] is itself a batch-layout buffer.  Each band of each native ROI equals,
 * bit for bit, what the fused kernel of prad_swt_level1_any_dev gives for the padded box.
 * verdict HOST int [B]: 0 the ROI was computed here; 8 it must be served by the single route (a padded extent -- n + (n & 1)
 * -- below flen, the condition of the fused single kernel; or a box above 2^31 - 1 voxels): its slice of `out` is not touched.
 * flen must be 2, 4 or 6 (haar / db1, db2 / sym2, coif1 / db3 / sym3): any other length in [2, 32] is PRAD_E_UNSUPPORTED with
 * nothing launched and nothing written; outside [2, 32] PRAD_E_ARG.  PRAD_E_ARG also for a NULL pointer, B < 1, a size < 1, a
 * negative offset, off[b] before the end of ROI b - 1, band_stride before the end of the last box, a dtype outside the list.
 * One copy (the record and item tables) and one launch on `stream`, which is then synchronised; no atomics, no memset; kernel
 * family "batch_swt" (prad_last_kernel_ms), prad_last_path "batch", prad_last_variant "batch-swt-fused".
 * prad_batch_swt_plan (host only, pure, needs no device): the planner the call itself uses.  verdict as above; *n_items = the
 * workgroups of the launch; items (may be NULL; int [*n_items][8], size it with a first call) = per workgroup ROI, z0, z1, y0,
 * y1, x0, x1 (half-open ranges clipped to the box) and the tile width TX (8, 16 or 32; TY = 256 / TX).  The items of a native
 * ROI tile its box exactly once; other ROIs get none.  Same argument errors as the call. */
int prad_batch_swt_plan(const int *sizes, int B, int flen, int *verdict, long long *n_items, int *items);
int prad_batch_swt_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, const double *dec_lo,
                       const double *dec_hi, int flen, double *out, long long band_stride, int *verdict, void *stream);

/* ---- the Laplacian-of-Gaussian images of many small boxes (csrc/kernels_batch_log.h) -----------------------------------
 * prad_batch_log_dev: ITK's LaplacianRecursiveGaussianImageFilter (NormalizeAcrossScale = normalize != 0) on each of B boxes
 * ALONE, for S sigmas, one workgroup per (ROI, sigma) pair and the whole filter of a box inside one compute unit's LDS -- per
 * ROI and sigma, bit for bit, what prad_log_multi_dev[_f64] gives for the box.  `in` (DEVICE) holds the boxes in the batch
 * layout of prad_batch_firstorder_dev, in the image's own dtype (0 float32, 1 float64, 2 int32, 3 int16; the derivative pass
 * of every term reads it widened to float64: exact); sizes ([B][3], z y x), off (element offsets, ascending, boxes not
 * overlapping), spacing ([B][3], z y x, per ROI) and the S sigmas (1 <= S <= 8, in the units of spacing) are HOST arrays.
 * out DEVICE [S][row_stride], float64 for dtype 1 and float32 otherwise, row_stride >= off[B - 1] + its voxels: the image of
 * ROI b for sigmas[s] lies at out + s * row_stride + off[b] in the box's own shape -- every row is a batch-layout buffer.
 * verdict HOST int [S][B]: 0 the pair was computed here; 8 the box is too large for the kernel -- an extent above 64, or
 * 4 Nz Ny (Nx | 1) bytes (the float32 image with an odd row pitch) above the 160 KiB of a compute unit's LDS: 32^3 fits, 36^3
 * does not -- and the single route (which asks the reference's question below itself) must serve the pair; 16 the reference
 * yields NO IMAGE for the pair (imageoperations.py getLoGImage: an extent below 4, or below ceil(sigma / spacing) + 1).  The
 * slice of `out` of a pair that is not 0 is never touched.
 * The native ROIs are sorted into at most three classes by their LDS footprint (<= 16 KiB, <= 64 KiB, above); a class is one
 * launch with the dynamic LDS of its largest ROI and 256, 512 or 768 lanes per workgroup.  One copy (the record, item and
 * coefficient tables) and up to three launches on `stream`, which is then synchronised; no atomics, no memset; kernel family
 * "batch_log" (prad_last_kernel_ms), prad_last_path "batch", prad_last_variant "batch-log".
 * PRAD_E_ARG, before anything is launched: a NULL pointer, B < 1, S outside [1, 8], a size < 1, a sigma <= 0, a spacing <= 0,
 * a negative offset, off[b] before the end of ROI b - 1, row_stride before the end of the last box, a dtype outside the list.
 * prad_batch_log_plan (host only, pure, needs no device): the planner the call itself uses.  verdict as above; lds_class HOST
 * int [B]: the class (0, 1, 2) of a ROI inside the kernel's domain, -1 for any other; *n_items = the workgroups of the call =
 * the zeros of verdict.  Same argument errors as the call. */
int prad_batch_log_plan(const int *sizes, int B, const double *spacing, const double *sigmas, int S, int *verdict,
                        int *lds_class, long long *n_items);
int prad_batch_log_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, const double *spacing,
                       const double *sigmas, int S, int normalize, void *out, long long row_stride, int *verdict, void *stream);

/* ---- the intensity transforms and the Gradient magnitude of many small boxes (csrc/kernels_batch_intensity.h) ---------------
 * prad_batch_intensity_dev: the image types Square, SquareRoot, Logarithm, Exponential and Gradient of the reference
 * (imageoperations.py:973-1091) on each of B boxes ALONE, in at most TWO launches for all boxes and all requested types.
 * `in` (DEVICE) holds the boxes in the batch layout of prad_batch_firstorder_dev, in the image's own dtype (0 float32,
 * 1 float64, 2 int32, 3 int16; widened to float64: exact); sizes ([B][3], z y x), off (element offsets, ascending, boxes not
 * overlapping) and spacing ([B][3], z y x, per ROI; NULL = 1 everywhere; read for Gradient with gradientUseSpacing != 0 only)
 * are HOST arrays.  types: bit 0 square, 1 squareroot, 2 logarithm, 3 exponential, 4 gradient.
 * out64 DEVICE float64 [rows][row_stride], one row per requested pointwise type in the order of the bits, row_stride >=
 * off[B - 1] + its voxels: the image of ROI b lies at out64 + row * row_stride + off[b] in the box's own shape -- every row is a
 * batch-layout buffer.  With top = max |x| over the BOX: square (x / sqrt(top))^2 as (c x)(c x), c = 1 / sqrt(top); squareroot
 * sign(x) sqrt(|x| top); logarithm (sign(x) log(|x| + 1)) (top / log(top + 1)); exponential exp((log(top) / top) x) -- float64,
 * no contraction, the operations of the single route in their order.  out_grad DEVICE float32 [off[B - 1] + its voxels]: per
 * axis z, y, x of extent > 1 the central difference 0.5 (x[i + 1] - x[i - 1]) with the neighbours clamped to the box (the box's
 * own edge is replicated), times 1 / spacing[axis] rounded on the host (with gradientUseSpacing), squared and summed in that
 * order in float64; the root rounded once to float32.  out64 / out_grad may be NULL when no bit asks for them.
 * verdict HOST int [B]: 0 the ROI was computed here; 1 top == 0 (the reference's formulas divide by zero): no pointwise row of
 * the ROI is written, its Gradient -- all zeros -- is; 2 a float box holds a NaN or an infinity: the caller fills every
 * requested image of the ROI from the single route.  With a pointwise type a launch of one workgroup per ROI works out top,
 * the constants and the verdicts, and the image launch writes nothing for a ROI of verdict 2; Gradient ALONE is ONE launch, which
 * finds such a ROI itself -- its slice of out_grad is then written (NaN where the arithmetic gives NaN) and must be replaced.
 * One copy (the record and item tables), the launches and one read-back (the verdicts) on `stream`, which is then synchronised;
 * no atomics, no memset; kernel family "batch_intensity" (prad_last_kernel_ms), prad_last_path "batch", prad_last_variant
 * "batch-intensity" ("batch-gradient" for Gradient alone).  B = 0 is a valid call that launches nothing.  Boxes are not capped.
 * PRAD_E_ARG, before anything is launched: a NULL pointer, B < 0, types outside [1, 31], a size < 1, a spacing that is read and
 * is not > 0 and finite, a negative offset, off[b] before the end of ROI b - 1, row_stride before the end of the last box, a dtype
 * outside the list.  PRAD_E_UNSUPPORTED: more than 16 777 215 ROIs or workgroups (about 1.7e10 voxels) in one call.
 * prad_batch_intensity_plan (host only, pure, needs no device): the planner the call itself uses.  *n_items = the workgroups
 * of the image launch; items (may be NULL; int64 [*n_items][4], size it with a first call) = per workgroup the half-open range
 * [w0, w1) of the batch's voxels in their packed order (voxel w of the batch is element w - sum of the voxels of the boxes before
 * its own of that box) and the first and last ROI the range touches; a workgroup writes its voxels of every requested row.  The
 * ranges tile [0, W) exactly once.  grid HOST int64 [2]: the workgroups of the two launches (grid[0] = 0 for Gradient alone).
 * Same argument errors as the call. */
int prad_batch_intensity_plan(const int *sizes, int B, int types, long long *n_items, long long *items, long long *grid);
int prad_batch_intensity_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, int types,
                             const double *spacing, int gradientUseSpacing, double *out64, long long row_stride, float *out_grad,
                             int *verdict, void *stream);

/* ---- resampling many small boxes, each onto a grid of its own (csrc/kernels_batch_resample.h) ------------------------------
 * prad_batch_mask_boxes_dev: mask (DEVICE, uint8, non-zero = ROI) holds B boxes in the batch layout; sizes ([B][3], z y x) and
 * off (element offsets) are HOST arrays.  boxes HOST int [B][7]: lo z / y / x, hi z / y / x (inclusive) and the voxel count of
 * every ROI; an empty mask gives count 0 (lo = the sizes, hi = -1).  One copy, ONE launch (a workgroup per ROI), one read-back
 * of 28 B bytes on `stream`, which is synchronised; kernel family "batch_mask_boxes", prad_last_variant "batch-mask-boxes".
 * prad_batch_resample_dev: prad_resample_dev on each of B boxes ALONE -- output voxel o of ROI b along axis d reads the box at
 * the continuous index start[b][d] + o * step[b][d] (the product rounded before the sum); interp[b] 0 nearest, 1 linear,
 * 3 cubic B-spline (the coefficients of the BOX, mirror boundaries at its faces) -- bit for bit what prad_resample_dev returns
 * for the box.  `in` (DEVICE): the boxes in the batch layout in the image's dtype (0 float32, 1 float64, 2 int32, 3 int16);
 * mask (DEVICE uint8, or NULL with out_mask NULL): the masks in the same layout, resampled nearest-neighbour on the same grid
 * in the same launch.  sizes, off, start ([B][3]), step ([B][3]), newsize ([B][3]), interp ([B]), out_off ([B], ascending,
 * outputs not overlapping) are HOST arrays in z y x order.  out (DEVICE, dtype of `in`; integer types are clamped to their
 * range, then truncated) and out_mask receive ROI b at element out_off[b] in the shape newsize[b]; 0 outside the box.
 * verdict HOST int [B]: 0 resampled here; 8 the box holds more than prad_batch_resample_max_vox() voxels (=
 * prad_batch_max_vox()) and prad_resample_dev must serve it -- its output slice is not touched.  Output voxels are not capped.
 * One copy and at most TWO launches whatever B is (the prefilter of the B-spline boxes, one workgroup per box, x then y then z
 * pass; the evaluation, divided by output voxels) on `stream`, which is then synchronised; kernel family "batch_resample",
 * prad_last_path "batch", prad_last_variant "batch-resample".  B = 0 is a valid call that launches nothing.
 * PRAD_E_ARG, before anything is launched: a NULL pointer, B < 0, a size or newsize < 1, a start or step that is not finite,
 * an interpolator outside {0, 1, 3}, a negative offset, out_off[b] before the end of ROI b - 1, a dtype outside the list, a mask
 * without out_mask or the reverse. */
int prad_batch_resample_max_vox(void);
int prad_batch_mask_boxes_dev(const uint8_t *mask, const int *sizes, const long long *off, int B, int *boxes, void *stream);
int prad_batch_resample_dev(const void *in, int dtype, const uint8_t *mask, const int *sizes, const long long *off, int B,
                            const double *start, const double *step, const int *newsize, const int *interp,
                            const long long *out_off, void *out, uint8_t *out_mask, int *verdict, void *stream);

/* ---- resegmentation on the device (radiomics/imageoperations.py:533-640 resegmentMask; csrc/kernels_resegment.h) ------------
 * The ROI is restricted to the voxels x with t0' <= x (one threshold) or t0' <= x <= t1' (two), [t0, t1] = sorted(range):
 * mode 0 absolute t' = t; 1 relative t' = top * t, top = the ROI's maximum; 2 sigma t' = mu + sd * t, mu the ROI's mean and sd
 * its population standard deviation.  The products are NOT sorted again: a negative maximum gives a descending pair, which keeps
 * nothing.  The arithmetic is numpy's on the host arrays for thresholds given as Python numbers: int16 / int32 / float64 images
 * are compared in float64; float32 images in float32 -- the bound is rounded to float32 first, and a relative bound is ONE
 * float32 product of the maximum and the rounded number.  The sum of an integer image is an exact 64-bit integer and its mean
 * one float64 division; every floating-point sum has one fixed order (no floating-point atomics; counts and boxes use integer
 * atomics), so the thresholds depend on the data alone and two calls give the same bits.
 * prad_resegment_dev: image (DEVICE; dtype 0 float32, 1 float64, 2 int32, 3 int16) and labelmap (DEVICE; label_dtype 2 int32,
 *   3 int16, 4 uint8, the codes of prad_label_census_dev) are C-contiguous arrays [size[0]]..[size[Nd-1]], Nd = 1..3; size and
 *   the nrange (1 or 2) values of range are HOST arrays.  out_mask (DEVICE, the label map's dtype and shape): `label` in the kept
 *   ROI, 0 everywhere else -- voxels of other labels included; every element is written.  HOST outputs: counts int64 [2] = ROI
 *   voxels on entry and kept; box int [6] = lo z / y / x, hi z / y / x of the kept ROI, inclusive (leading axes of an array with
 *   Nd < 3 have extent 1; nothing kept: lo = the sizes, hi = -1); thr float64 [2] = the thresholds (thr[1] = +inf with one).
 *   At most THREE launches -- absolute: initialisation and mask; relative: maximum and mask; sigma: count and sum, squared
 *   deviations about the mean (as np.std is defined), mask -- and ONE read-back of 64 bytes on `stream`, which is synchronised.
 *   Work is divided by voxels over a grid that follows from the voxel count alone; 64-bit indices.  Kernel family "resegment"
 *   (prad_last_kernel_ms), prad_last_path "resegment", prad_last_variant "resegment-absolute" / "-relative" / "-sigma".
 *   PRAD_E_UNSUPPORTED: sigma mode on a float32 image (numpy accumulates its mean in float32; nothing is launched); a NaN or an
 *   infinity inside the ROI (found by the launches: out_mask is then not valid) -- the host code serves both.  PRAD_E_ARG, before
 *   anything is launched: a NULL pointer, a dtype or mode outside the lists, nrange outside [1, 2], a NaN in range, Nd outside
 *   [1, 3], a size < 1.
 * prad_batch_resegment_dev: the same for B boxes in the batch layout of prad_batch_firstorder_dev (image in its own dtype, uint8
 *   mask, non-zero = ROI; HOST sizes [B][3] / off), one mode and range for all of them, in ONE launch -- a workgroup per ROI walks
 *   its box once per pass -- and one read-back.  out_mask DEVICE uint8, the batch layout: 1 in the kept ROI, 0 elsewhere.  HOST
 *   outputs: boxes int [B][7] in the layout of prad_batch_mask_boxes_dev (box and count of the KEPT ROI), thr float64 [B][2],
 *   verdict int [B]: 0 fine; 1 the ROI is empty on entry; 2 a non-finite value inside the ROI; 3 at most one voxel kept (boxes
 *   still holds the count); 8 not served here -- a box above prad_batch_max_vox() voxels (the cap only keeps one workgroup's walk
 *   short: the kernel keeps no copy of the box) or sigma mode on float32 -- the slice of out_mask is not touched.  Verdicts 1 and 2
 *   write an all-zero mask.  A ROI's row depends on its values alone, not on its place in the batch or on the other ROIs.  Kernel
 *   family "batch_resegment", prad_last_path "batch", prad_last_variant "batch-resegment".  B = 0 is a valid call that launches
 *   nothing.  PRAD_E_ARG as above, and for B < 0, a negative offset. */
int prad_resegment_dev(const void *image, int dtype, const void *labelmap, int label_dtype, const int *size, int Nd, int label,
                       int mode, const double *range, int nrange, void *out_mask, long long *counts, int *box, double *thr,
                       void *stream);
int prad_batch_resegment_dev(const void *image, int dtype, const uint8_t *mask, const int *sizes, const long long *off, int B,
                             int mode, const double *range, int nrange, uint8_t *out_mask, int *boxes, double *thr, int *verdict,
                             void *stream);

/* ---- filter stack in front of the matrices (radiomics/imageoperations.py:756-970) ---------------------------
 * The arithmetic of both filters lives in third-party wheels (PyWavelets, SimpleITK/ITK) that are not part of
 * the reference tree; these entry points implement their published algorithms (see oracle/filters_oracle.py):
 * parity is pinned by the 198 brain1 values the reference recorded in notebooks/helloFeatureClass.ipynb
 * (tests/test_notebook_pin.py).
 *
 * prad_swt_level1: one level of the undecimated (stationary) wavelet transform with periodisation along `axes`
 * (in that order), i.e. pywt.swtn(data, wavelet, level=1, start_level=0, axes) (imageoperations.py:928,935).
 *   in   float64 [size[0]]..[size[Nd-1]], every transformed axis of even length
 *   out  float64 [2^naxes][...]: sub-bands in PyWavelets' key order ('a' = dec_lo before 'd' = dec_hi, the first
 *        axis of `axes` is the most significant letter): aaa, aad, ada, add, daa, dad, dda, ddd for 3 axes.
 * prad_log: ITK LaplacianRecursiveGaussianImageFilter (imageoperations.py:824-830): float32 in / out; per dimension the
 *   second-order pass along it first, then the zero-order passes along the other dimensions in increasing ITK direction
 *   (the order that reproduces the float32 order statistics the reference recorded for brain1 bit for bit),
 *   `spacing` per ARRAY axis (i.e. SimpleITK spacing reversed), sigma in the units of spacing,
 *   normalize != 0 multiplies by sigma^2 (NormalizeAcrossScale).  Every axis needs >= 4 samples. */
int prad_swt_level1(const double *in, const int *size, int Nd, const double *dec_lo, const double *dec_hi, int flen,
                    const int *axes, int naxes, double *out);
int prad_swt_level1_dev(const double *in, const int *size, int Nd, const double *dec_lo, const double *dec_hi,
                        int flen, const int *axes, int naxes, double *out, void *stream);
/* The same with the image in its own element type (dtype codes as prad_roi_minmax_dev: 0 float32, 1 float64, 2 int32,
 * 3 int16): the widening to float64 is folded into the fused 3-D kernel.  (The reference copies and pads the array,
 * imageoperations.py:914-919, and pywt.swtn widens integer images to float64; it keeps FLOAT32 images in float32 arithmetic
 * and returns float32 sub-bands -- here every input type is transformed in float64: for float32 images the sub-bands carry
 * more precision than the reference's, a stated deviation)
 * PRAD_E_UNSUPPORTED when the call is not a 3-D transform over axes (2, 1, 0) with 2 / 4 / 6 taps: convert and use
 * prad_swt_level1_dev. */
int prad_swt_level1_any_dev(const void *in, int dtype, const int *size, int Nd, const double *dec_lo,
                            const double *dec_hi, int flen, const int *axes, int naxes, double *out, void *stream);
int prad_log(const float *in, const int *size, int Nd, const double *spacing, double sigma, int normalize,
             float *out);
int prad_log_dev(const float *in, const int *size, int Nd, const double *spacing, double sigma, int normalize,
                 float *out, void *stream);
/* nsig (1..8) sigmas of ONE input in the same launches (the reference loops over its sigma list, imageoperations.py:
 * 806-836, one filter run each): a pass of one sigma is bound by the latency of its serial recursion, the waves of the
 * other sigmas fill the gaps.  outs: HOST array of nsig DEVICE pointers; the same arithmetic per sigma as prad_log_dev. */
int prad_log_multi_dev(const float *in, const int *size, int Nd, const double *spacing, const double *sigmas, int nsig,
                       int normalize, float *const *outs, void *stream);
/* The same filter on float64 images (e.g. after `normalize: true`, whose output is float64): the result is float64 like the
 * input (sitk.LaplacianRecursiveGaussianImageFilter keeps the pixel type, imageoperations.py:824-830) and is computed as
 * ITK computes it: the derivative pass of every term reads the float64 input, the images between the passes and the
 * cumulative image are float (itkLaplacianRecursiveGaussianImageFilter.h: InternalRealType = float), the sum is widened at
 * the end.  (Rounds 3-4 kept float64 images between the passes.) */
int prad_log_f64(const double *in, const int *size, int Nd, const double *spacing, double sigma, int normalize,
                 double *out);
int prad_log_dev_f64(const double *in, const int *size, int Nd, const double *spacing, double sigma, int normalize,
                     double *out, void *stream);
int prad_log_multi_dev_f64(const double *in, const int *size, int Nd, const double *spacing, const double *sigmas,
                           int nsig, int normalize, double *const *outs, void *stream);

/* ---- LBP2D: local binary patterns by plane (csrc/kernels_lbp2d.h, csrc/kernels_batch_lbp2d.h) ----------------------------------
 * The image type LBP2D of the reference (imageoperations.py:1094-1166 on scikit-image's local_binary_pattern, whose arithmetic
 * is restated in csrc/kernels_lbp2d.h and DESIGN.md "LBP2D": float64, every product and sum rounded, nothing fused).
 * prad_lbp2d_dev: ONE launch for the volume `in` (DEVICE, dtype code 0 float32, 1 float64, 2 int32, 3 int16) of extents
 * size[3] = (nz, ny, nx) -- a 2-D image is (1, ny, nx) with axis 0 --, planes stacked along `axis` (force2Ddimension: 0 rows y
 * cols x, 1 rows z cols x, 2 rows y cols z).  rp, cp HOST float64 [P]: the row and column offset of every sample, computed by
 * the caller (round(-R sin(2 pi i / P), 5), round(R cos(2 pi i / P), 5)); halo = ceil(R), and every |rp|, |cp| <= halo.
 * method: 0 uniform, 1 default, 2 ror.  out (DEVICE, not `in`): the codes in the image's own dtype.  The call only enqueues on
 * `stream`.  PRAD_E_UNSUPPORTED (nothing launched; the caller takes its host route) for P > 24, halo > 8 or more than 2^31 - 1
 * tiles; PRAD_E_ARG for an extent below 1, an axis outside 0 .. 2, P < 1, a sample beyond the halo, an unknown method or
 * dtype, in == out, and default / ror codes of more than 15 samples into an int16 image.
 * prad_lbp2d_plan (host only, pure, needs no device): the plan the call executes.  tile int [3]: the output voxels (tz, ty, tx)
 * of a workgroup; grid int64 [4]: the tiles along z, y, x and their product, the workgroups of the launch; *lds_bytes: the
 * dynamic LDS of a workgroup (at most 40 KiB); *verdict: 0 native, 1 halo outside [0, 8], 2 too many workgroups.
 * prad_batch_lbp2d_dev: the same images for B boxes ALONE (cells beyond a box's edge read 0.0) in ONE launch, boxes of any size,
 * in the batch layout of prad_batch_firstorder_dev (sizes HOST int [B][3], off HOST int64 [B], boxes following one another);
 * out DEVICE float64, box b at out + off[b]: bit for bit what prad_lbp2d_dev writes for the box, widened.  Same statuses.
 * prad_batch_lbp2d_plan: one tile shape per launch, that of the largest extent per axis; *n_items workgroups; items (may be
 * NULL; int [*n_items][4], size it with a first call) = per workgroup the ROI and the first output voxel (z0, y0, x0) of its
 * tile inside the box. */
int prad_lbp2d_plan(const int *size, int axis, int halo, int *tile, long long *grid, long long *lds_bytes, int *verdict);
int prad_lbp2d_dev(const void *in, int dtype, const int *size, int axis, const double *rp, const double *cp, int P, int halo,
                   int method, void *out, void *stream);
int prad_batch_lbp2d_plan(const int *sizes, int B, int axis, int halo, int *tile, long long *n_items, int *items,
                          long long *lds_bytes, int *verdict);
int prad_batch_lbp2d_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, int axis, const double *rp,
                         const double *cp, int P, int halo, int method, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PYRADIOMICS_AMD_H */
