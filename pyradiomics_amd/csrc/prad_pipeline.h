// prad_pipeline.h -- the executor of the deferred GLCM + GLRLM pipeline (a textual part of prad_api.hip, inside its anonymous
// namespace: the texture kernels stay in one unit).  What a call or a flush launches is decided by prad_pipe_plan.h,
// whose header comment describes the pipeline, its workspace sets and twin; the functions here ask the planner for a record, map
// its (set, range) names to pointers, launch, record events -- and decide nothing about sets or zeroing themselves.
//
// Across the two instances nothing is shared on the device except
//   * the sticky verdict word, which every writer only ever SETS (the finalize kernels, the latch kernels); only
//     prad_deferred_status clears it, after it has synchronised both streams;
//   * output buffers a caller hands to calls on BOTH instances: each instance remembers the output ranges of what it has in flight
//     (PipeState::outs); a call whose outputs overlap a range of the other instance first flushes that instance and lets its own
//     stream wait for it (an event), so the later call's values stand last, as on one stream.
// A change of an instance's stream (a twin call behind one that was not, or the reverse; a caller with two streams) is ordered
// with an event.  Every drain (join, status, mark, mode / lanes / device changes, workspace release, a volume the pipeline does
// not take) covers both instances.
//
// The switches (SweepKnobs) are read afresh on every call and every flush, so that a test can flip PRAD_FIN_RIDE=0 (the finalize
// of a pipeline volume as a launch of its own behind its walk launch, zero3_kernel in front of every pack: A/B, and the checker
// of the riding job) or PRAD_FINALIZE_ONE=0 (the three finalize launches instead of finalize_volume_kernel) inside one process.
//
// Included by prad_api.hip only, inside its anonymous namespace, behind zero3_kernel (prad_pipe_plan.h: at the top of that unit).

// One packed volume between its pack and its finalize: device pointers of ONE workspace set (Context::lane) and the plan.
struct VolState {
  SweepPlan p;
  int Ng = 0, Nr = 0, Na = 0;
  double *glcm = nullptr, *glrlm = nullptr;   // outputs (device), either may be NULL
  uint8_t *levels = nullptr, *rowzero = nullptr;
  uint8_t *levels16 = nullptr;   // 16-bit level*4 elements (two-table fixed-window kernel)
  u32 *acc = nullptr, *glcm_acc = nullptr, *glrlm_acc = nullptr;
  int *multi = nullptr;
  int *flags_d = nullptr;
};
// What a volume needs zeroed: accumulators + control words (before its WALKS), row flags and flag words (before its PACK);
// indexed by kZeroAcc, kZeroRz, kZeroFl.
struct ZeroNeed {
  u32 *p[3] = {nullptr, nullptr, nullptr};
  size_t w[3] = {0, 0, 0};
};
// ONE launch (three hipMemsetAsync calls are three launches, each with its dependent-launch gap on the stream)
int launch_zero3(hipStream_t s, const ZeroNeed &z) {
  const size_t total_w = z.w[0] + z.w[1] + z.w[2];
  if (total_w == 0) return PRAD_OK;
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((total_w / 4 + 255) / 256, 1024));
  hipLaunchKernelGGL(zero3_kernel, dim3(gx), dim3(256), 0, s, z.p[0], z.w[0], z.p[1], z.w[1], z.p[2], z.w[2]);
  return check_launch("zero3_kernel");
}

// (prad_api.hip, below the pipeline)
int vol_prepare(Call &k, const SweepPlan &p, int Ng, int Nr, double *glcm, double *glrlm, VolState &v, ZeroNeed &z);
int vol_pack_standalone(Call &k, VolState &v);
int vol_sweep(Call &k, const SweepKnobs &kn, const VolState &v, const PackJob &pj, const FinJob &fj);
int vol_finalize(Call &k, const SweepKnobs &kn, const VolState &v, int *sticky);

bool pipeline_volume(const SweepPlan &p, bool glcm, bool glrlm) {   // a volume the two-stage deferred pipeline takes
  if (!(p.ok && p.lines.count > 0 && glcm && glrlm)) return false;
  return (p.fw && p.fused) || p.fw2;
}
// can this volume's pack ride in another volume's sweep launch?  (linear layout, vector loads)
bool pack_inline_ok(const Call &k, const VolState &v) {
  if (!(v.glcm && v.glrlm && v.p.pitch == v.p.Nx && v.p.padw == 0 && (k.g.n % 16) == 0 &&
        ((((uintptr_t)k.image) | ((uintptr_t)k.mask) | ((uintptr_t)v.levels)) & 15) == 0))
    return false;
  // (PackWave16 keeps its piece's voxel index in 32 bits, PackWave its row-flag index: side-job packs stay below 2^31 voxels --
  //  ADVICE r5; a larger volume packs in a launch of its own)
  if (k.g.n >= (1LL << 31)) return false;
  if (v.p.fw2) return v.levels16 && v.p.pitch16 == 2 * v.p.Nx && (((uintptr_t)v.levels16) & 15) == 0;
  return v.p.fw && v.p.fused;
}

PackJob make_pack_job(const Call &k, const SweepKnobs &kn, const VolState &v, const VolState &host) {
  PackJob j;
  memset(&j, 0, sizeof(j));
  j.image = k.image;
  j.mask = k.mask;
  j.levels = v.levels;
  j.levels16 = v.p.fw2 ? v.levels16 : nullptr;
  j.rowzero = v.rowzero;
  j.flags = v.flags_d;
  j.n16 = k.g.n / 16;
  j.NX = v.p.Nx;
  j.Ng = v.Ng;
  // cadence: spread a wave's units over the plain groups of its walk (both per wave); what is left drains behind the walk
  double groups = 0;
  for (int i = 0; i < host.p.fwset.count; i++) groups += (double)host.p.fwset.d[i].NM * host.p.fwset.d[i].NU / PRAD_FW_U;
  const double units = (double)j.n16 / 64.0;
  // (two-table walk: a unit every 3rd group instead of every 2nd at 512^3 -- 0.707 -> 0.698 ms per volume, smooth inside its run-to-run spread of 0.75 - 0.78;
  //  the fused-table walk measures best at 2: 0.490 against 0.496 at 3, profiles/r05b_probes.md)
  const double slack = v.p.fw2 ? 1.05 : 0.92;
  j.every = (int)std::max(1.0, std::min(64.0, std::floor(slack * groups / std::max(1.0, units))));
  if (kn.pack_every.set) j.every = std::max(1, (int)kn.pack_every.v);
  return j;
}

struct OutRange {
  const char *lo, *hi;
};
struct PipeState {   // what one instance has in flight: the planner (PipePlanner::pending, walked) says which of the two volumes are
  VolState pending;
  VolState walked;              // walked, not finalized: its finalize rides in the next walk launch or runs stand-alone first
  hipStream_t s = nullptr;      // stream the pending volume's pack was enqueued on
  hipEvent_t ev = nullptr;
  std::vector<OutRange> outs;   // outputs of calls enqueued since the instance was last waited for by the host or by the other one
};
struct Pipelines {
  PipePlanner plan;
  PipeState ex[kPipes];
  int mode = -1;                // 1 pipeline, 0 lanes
};
Pipelines &pipelines() {
  static thread_local Pipelines p;
  return p;
}
bool pipeline_mode(const SweepKnobs &kn) {
  Pipelines &P = pipelines();
  if (P.mode < 0) P.mode = kn.lanes_mode ? 0 : 1;
  return P.mode == 1;
}
bool pipelines_busy() { return pipe_busy(pipelines().plan); }
// nothing in flight and nothing known to be zero any more (the workspace goes away); device_changes: the streams and events too
void pipelines_forget(bool device_changes) {
  Pipelines &P = pipelines();
  pipe_forget(P.plan);
  for (int i = 0; device_changes && i < kPipes; i++) {
    P.ex[i].s = nullptr;
    P.ex[i].ev = nullptr;
    P.ex[i].outs.clear();
  }
}
// `s` waits (on the device) for everything the instance has enqueued on a stream of its own
int pipeline_order(PipeState &ps, hipStream_t s) {
  if (!ps.s || ps.s == s) return PRAD_OK;
  if (!ps.ev) PRAD_HIP(hipEventCreateWithFlags(&ps.ev, hipEventDisableTiming));
  PRAD_HIP(hipEventRecord(ps.ev, ps.s));
  PRAD_HIP(hipStreamWaitEvent(s, ps.ev, 0));
  return PRAD_OK;
}
void out_ranges_add(PipeState &ps, const double *glcm, size_t nglcm, const double *glrlm, size_t nglrlm) {
  const OutRange r[2] = {{(const char *)glcm, (const char *)(glcm + nglcm)}, {(const char *)glrlm, (const char *)(glrlm + nglrlm)}};
  for (int i = 0; i < 2; i++) {
    if (!r[i].lo) continue;
    bool known = false;
    for (OutRange &o : ps.outs)
      if (o.lo <= r[i].lo && r[i].hi <= o.hi) known = true;
    if (known) continue;
    if (ps.outs.size() >= 64) {   // (a caller with ever new buffers: one range that covers them all -- overlaps may be reported that are none)
      for (const OutRange &o : ps.outs) {
        ps.outs[0].lo = std::min(ps.outs[0].lo, o.lo);
        ps.outs[0].hi = std::max(ps.outs[0].hi, o.hi);
      }
      ps.outs.resize(1);
    }
    ps.outs.push_back(r[i]);
  }
}
bool out_ranges_overlap(const PipeState &ps, const double *glcm, size_t nglcm, const double *glrlm, size_t nglrlm) {
  const OutRange r[2] = {{(const char *)glcm, (const char *)(glcm + nglcm)}, {(const char *)glrlm, (const char *)(glrlm + nglrlm)}};
  for (int i = 0; i < 2; i++)
    for (const OutRange &o : ps.outs)
      if (r[i].lo && r[i].lo < o.hi && o.lo < r[i].hi) return true;
  return false;
}

bool fin_job_empty(const FinJob &fj) { return fj.Na == 0 && fj.zn[0] + fj.zn[1] + fj.zn[2] == 0; }

// can the finalize of pipeline volume v ride in a walk launch?  (the conditions of the one-launch finalize, a walk launch that is
// the volume's last, and the job's 32-bit element indices)
bool fin_can_ride(const SweepKnobs &kn, const VolState &v) {
  const SweepPlan &p = v.p;
  if (!(v.glcm && v.glrlm && p.fw && p.fused && p.lines.count > 0 && v.levels)) return false;
  if (p.row_slot >= 0 && p.fw_xblocks == 0) return false;   // (PRAD_FW_XROLE=0: the x angle is a launch behind the walk launch)
  if (!kn.finalize_one || (long long)v.Ng * v.Nr >= (1LL << 30) || v.Ng > 255 || v.Na > PRAD_MAX_SWEEP || v.Na != p.aset.count) return false;
  return ((long long)v.Ng * v.Nr + (long long)v.Ng * v.Ng) * v.Na < (1LL << 31);
}
// can the walk launch of `host` on stream s carry a FinJob?  (with or without a pack job)
bool fin_host_ok(const SweepKnobs &kn, const PipeState &ps, const VolState &host, hipStream_t s) {
  const SweepPlan &p = host.p;
  if (!(kn.fin_ride && ps.s == s && host.glcm && host.glrlm && p.fw && p.fused && p.lines.count > 0)) return false;
  const size_t lds = p.fw_xblocks > 0 ? std::max(p.lds_fw, p.lds_fw_rows) : p.lds_fw;   // (as launch_fw_kpp)
  return lds >= (size_t)PRAD_FIN_SCRATCH_BYTES && p.fw_blocks >= 1 && p.fw_blocks < 32768;
}

// The riding job of walk launch L of `host`: the finalize of `walked` (or none) and the zeroing the planner named, each range the
// buffer that the book knows for (set, kind of range).
FinJob make_fin_job(const PipePlanner &pl, const PipeLaunch &L, const VolState &host, const VolState *walked, int *sticky) {
  FinJob j;
  memset(&j, 0, sizeof(j));
  if (!L.job) return j;
  const int nline = host.p.fw_blocks;
  if (walked) {
    const VolState &w = *walked;
    j.Na = w.Na;
    j.Ng = w.Ng;
    j.Nr = w.Nr;
    j.Nz = w.p.Nz;
    j.Ny = w.p.Ny;
    j.Nx = w.p.Nx;
    j.pitch = w.p.pitch;
    j.L = w.levels;
    j.glcm_acc = w.glcm_acc;
    j.glrlm_acc = w.glrlm_acc;
    j.glcm_out = w.glcm;
    j.glrlm_out = w.glrlm;
    j.multi = w.multi;
    j.flags = w.flags_d;
    // Placement of the 13 angle workgroups (each starts its walk ~7 us late; the role's chunk hand-out makes up for it):
    // angle a on workgroup a / count of role a % count
    const FwSet &fs = host.p.fwset;
    for (int a = 0; a < w.Na; a++) {
      for (int d = 0; d < 3; d++) j.off[a][d] = (signed char)w.p.aset.off[a][d];
      const int role = a % fs.count, idx = a / fs.count;
      const int b = (fs.first_block[role] + idx < fs.first_block[role + 1]) ? fs.first_block[role] + idx : a % nline;
      j.ablock[a] = (short)b;
    }
  }
  for (int r = 0; r < 3; r++)
    if (L.z[r].set >= 0) {
      j.z[r] = reinterpret_cast<u32 *>(pl.book[L.z[r].set].id[r]);
      j.zn[r] = (unsigned)L.z[r].words;
    }
  j.sticky = sticky;
  return j;
}

// Carries out the launches of one step of instance i on stream s, in the planner's order.  pj: the new volume's pack as a side
// job of the walk launch (or n16 == 0); kv: the new volume and its call (a flush: none).
int pipeline_execute(Context &c, const SweepKnobs &kn, int i, hipStream_t s, const PipeStep &st, const PackJob &pj, Call *kv, VolState *v) {
  Pipelines &P = pipelines();
  PipeState &ps = P.ex[i];
  int *sticky = nullptr;
  PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
  Call k;   // the kernels of a volume in flight read its geometry from its VolState
  k.c = &c;
  bool walk_done = false, any_walk = false;
  for (int n = 0; n < st.n; n++) any_walk = any_walk || st.l[n].kind == kLaunchWalk;
  for (int n = 0; n < st.n; n++) {
    const PipeLaunch &L = st.l[n];
    if (L.kind == kLaunchZero3) {
      ZeroNeed z;
      for (int r = 0; r < 3; r++)
        if (L.z[r].set >= 0) {
          z.p[r] = reinterpret_cast<u32 *>(P.plan.book[L.z[r].set].id[r]);
          z.w[r] = L.z[r].words;
        }
      PRAD_TRY(launch_zero3(s, z));
    } else if (L.kind == kLaunchFinalize) {
      // in front of the walk launch: the walked volume (with nothing to walk, on the stream it was walked on); behind it: the pending one
      const VolState &f = walk_done ? ps.pending : ps.walked;
      k.s = any_walk ? s : ps.s;
      k.Na = f.Na;
      k.flags_d = f.flags_d;
      PRAD_TRY(vol_finalize(k, kn, f, sticky));
    } else if (L.kind == kLaunchWalk) {
      const FinJob fj = make_fin_job(P.plan, L, ps.pending, L.fin >= 0 ? &ps.walked : nullptr, sticky);
      k.s = s;
      k.Na = ps.pending.Na;
      k.flags_d = ps.pending.flags_d;
      PRAD_TRY(vol_sweep(k, kn, ps.pending, pj, fj));
      walk_done = true;
    } else {
      PRAD_TRY(vol_pack_standalone(*kv, *v));
    }
  }
  if (st.keep) ps.walked = ps.pending;
  return PRAD_OK;
}

// nothing pending or walked in the instance afterwards (kernels enqueued on the pending volume's own stream; no host
// synchronisation).  A failure leaves the instance empty: what could not be enqueued is not tried again.
int pipeline_flush(Context &c, const SweepKnobs &kn, int i) {
  Pipelines &P = pipelines();
  PipeState &ps = P.ex[i];
  if (!pipe_busy(P.plan, i)) return PRAD_OK;
  PackJob none;
  memset(&none, 0, sizeof(none));
  StepInput in;
  in.inst = i;
  in.host_ok = P.plan.pending[i] >= 0 && fin_host_ok(kn, ps, ps.pending, ps.s);
  in.walked_can_ride = P.plan.walked[i] >= 0 && fin_can_ride(kn, ps.walked);
  const PipeStep st = pipe_step(P.plan, in);
  const size_t before = c.times.size();
  const int rc = pipeline_execute(c, kn, i, ps.s, st, none, nullptr, nullptr);
  if (rc != PRAD_OK) pipe_abandon(P.plan, i);
  if (c.timing_accumulate) c.all_times.insert(c.all_times.end(), c.times.begin() + (long)before, c.times.end());
  return rc;
}
// ... both instances (every drain does; the first failure is reported, the other instance is flushed all the same)
int pipeline_flush(Context &c, const SweepKnobs &kn) {
  int rc = PRAD_OK;
  for (int i = 0; i < kPipes; i++) {
    const int r = pipeline_flush(c, kn, i);
    if (rc == PRAD_OK) rc = r;
  }
  return rc;
}
// ... from an entry point that is no GLCM / GLRLM call (join, mark, status, set_device, ...): it reads the switches itself, and
// only when there is a volume to flush
int pipeline_flush(Context &c) {
  if (!pipelines_busy()) return PRAD_OK;
  return pipeline_flush(c, sweep_knobs_from_env());
}
// `s` waits (on the device) for what both instances have enqueued on streams of their own
int pipelines_order(hipStream_t s) {
  for (int i = 0; i < kPipes; i++) PRAD_TRY(pipeline_order(pipelines().ex[i], s));
  return PRAD_OK;
}
// the host waits for both instances; afterwards none of their outputs is in flight
int pipelines_sync() {
  for (int i = 0; i < kPipes; i++) {
    PipeState &ps = pipelines().ex[i];
    if (ps.s) PRAD_HIP(hipStreamSynchronize(ps.s));
    ps.outs.clear();
  }
  return PRAD_OK;
}

// The instance, the stream and the workspace set (Context::lane) of a deferred whole-volume call in pipeline mode.  twin: the call
// goes to one of two pipelines on internal streams; else instance 0 on the caller's stream.
int pipeline_enter(Context &c, const SweepKnobs &kn, const int *size, int Nd, int Na, int Ng, int Nr, const double *glcm,
                   const double *glrlm, hipStream_t *s, int *inst) {
  Pipelines &P = pipelines();
  long long voxels = -1;
  if (size && Nd >= 1 && Nd <= PRAD_MAX_ND) {
    voxels = 1;
    for (int d = 0; d < Nd; d++) voxels *= std::max(size[d], 1);
  }
  const PipeChoice ch = pipe_choose(P.plan, kn.pipe_twin, voxels);
  if (ch.twin) {
    PRAD_TRY(c.twin_streams());
    PRAD_TRY(c.lane_enter(ch.inst, *s, s));
  } else {
    PRAD_TRY(pipeline_flush(c, kn, 1));   // (instance 1 holds volumes of twin calls only)
  }
  // an output buffer that the other instance still writes: that instance finishes first, and this call's stream waits for it
  PipeState &other = P.ex[1 - ch.inst];
  if (Na >= 1 && out_ranges_overlap(other, glcm, glcm ? (size_t)Na * Ng * Ng : 0, glrlm, glrlm ? (size_t)Na * Ng * Nr : 0)) {
    PRAD_TRY(pipeline_flush(c, kn, 1 - ch.inst));
    PRAD_TRY(pipeline_order(other, *s));
    other.outs.clear();
  }
  c.lane = ch.set;
  *inst = ch.inst;
  return PRAD_OK;
}

// one deferred call of a pipeline volume: its workspace, the step's launches, and the volume becomes the instance's pending one
int pipeline_step(Call &k, const SweepKnobs &kn, int i, const SweepPlan &p, int Ng, int Nr, double *glcm, double *glrlm) {
  Context &c = *k.c;
  Pipelines &P = pipelines();
  PipeState &ps = P.ex[i];
  // the instance changes its stream: the new stream waits for the old one before anything of this call -- its zeroing included
  // -- is enqueued
  PRAD_TRY(pipeline_order(ps, k.s));
  VolState v;
  ZeroNeed z;
  PRAD_TRY(vol_prepare(k, p, Ng, Nr, glcm, glrlm, v, z));
  const uintptr_t id[3] = {(uintptr_t)z.p[kZeroAcc], (uintptr_t)z.p[kZeroRz], (uintptr_t)z.p[kZeroFl]};
  const bool have = P.plan.pending[i] >= 0;
  StepInput in;
  in.inst = i;
  in.new_set = c.lane;
  in.need = pipe_prepare(P.plan, c.lane, id, z.w, v.rowzero ? c.bufs[c.key("rowzero")].cap : 0, kn.fin_ride);
  PackJob pj;
  memset(&pj, 0, sizeof(pj));
  // (the side job writes the layout of the launch it rides in: fused-table and two-table volumes do not mix)
  in.pack_inline = have && pack_inline_ok(k, v) && ps.pending.p.fw2 == v.p.fw2 && !kn.no_inline_pack;
  if (in.pack_inline) pj = make_pack_job(k, kn, v, ps.pending);
  in.host_ok = have && fin_host_ok(kn, ps, ps.pending, k.s);
  in.walked_can_ride = P.plan.walked[i] >= 0 && fin_can_ride(kn, ps.walked);
  in.pending_can_stay = have && kn.fin_ride && fin_can_ride(kn, ps.pending);
  const PipeStep st = pipe_step(P.plan, in);
  const int rc = pipeline_execute(c, kn, i, k.s, st, pj, &k, &v);
  if (rc != PRAD_OK) {
    pipe_abandon(P.plan, i);
    return rc;
  }
  ps.pending = v;
  ps.s = k.s;
  out_ranges_add(ps, glcm, (size_t)k.Na * Ng * Ng, glrlm, (size_t)k.Na * Ng * Nr);
  return PRAD_OK;
}
