// prad_pipe_plan.h -- the decisions of the deferred GLCM + GLRLM pipeline: which instance and workspace set a call gets, what
// still has to be zeroed for its volume, and what every launch of a step walks, packs, finishes and zeroes.  Pure functions of a
// per-thread PipePlanner and plain integers: no HIP type, no pointer, no launch.  Buffers are opaque ids with a capacity.
// prad_pipeline.h (the executor) asks for a record and carries it out; pipe_replay runs a script of events through a fresh planner
// for prad_debug_pipe_plan, and tests/test_pipe_plan.py holds the records to a model of the workspace without a device.
//
// The pipeline.  A deferred whole-volume call N launches { walks of volume N-1 + pack of volume N } as ONE fixed-window launch (the
// pack is a side job of the walking waves: kernels_sweepfw.h PackJob).  Volume N itself stays PENDING (packed, not yet walked)
// until the next deferred call or until prad_deferred_status / prad_deferred_join / prad_deferred_mark flush it.
//
// Fused-table volumes (<= 36 levels) go one stage further: volume N-1 is not finalized behind its walk launch but stays WALKED,
// and the NEXT walk launch -- the one of call N+1, which walks N and packs N+1 -- carries its finalize and the zeroing for the
// volumes to come as a riding job (FinJob), so a steady step is ONE launch: no zero3_kernel, no finalize_volume_kernel.  The
// job rides only in a fused-table launch on the same stream; otherwise (a two-table volume, another stream,
// PRAD_FW_XROLE=0, PRAD_FINALIZE_ONE=0, PRAD_FIN_RIDE=0, any flush) the stand-alone finalize of the walked volume is launched
// FIRST.  Every flush finishes the walked volume too, so the contract stands: outputs are valid after prad_deferred_status,
// prad_deferred_join or a mark.  The two-table route (40 - 170 levels) is finalized behind its walk launch.
//
// Workspace sets.  Three volumes are in flight -- packed, walked, being finalized (whose LEVELS the rare exact test reads) -- so
// FOUR sets alternate (set = first set of the instance + seq % 4).  Launch N walks N-1 (set N-1), packs N (set N), finalizes N-2
// (set N-2) and zeroes
//   * the accumulators and control words of set N: used by the walks of N in launch N+1, last read by the finalize of N-4;
//   * the row flags and the four flag words of set N+1 = set N-3: written by the pack of N+1 in launch N+1, last read in
//     launches N-2 (row flags, walks of N-3) and N-1 (flag words, finalize of N-3).
// A set remembers what is known to be zero (SetZero): pipe_prepare asks zero3_kernel only for the rest (the first volumes of a
// run, a grown buffer, more rows than were re-zeroed).  The INVARIANT that makes this safe is stated at pipe_step, which keeps it.
//
// Twin (PRAD_PIPE_TWIN; automatic from kTwinMinVoxels voxels).  All of the above is ONE instance.  There are two per thread.  A
// twin call n -- n counts the twin calls of the thread -- goes to instance n % 2, which runs on internal stream n % 2 and owns the
// workspace sets (n % 2) * 4 ... + 3.  Its launch { walk n-2, pack n, finalize n-4, zeroing } depends on launch n-2 only, so
// launches n and n+1 are unordered on the device and the line workgroups of n+1 take the CUs that come free at the uneven end of
// n.  "N-1" above reads "the instance's previous call".  The sets of the two instances are disjoint and no record names a set of
// the other instance, so the invariant holds per instance, and across instances there is nothing shared to order except the
// sticky verdict word and the callers' output buffers (prad_pipeline.h).  A call that is not twin runs on instance 0 on the
// caller's stream; instance 1 holds volumes of twin calls only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace prad {
#pragma GCC visibility push(hidden)   // (the library exports the C ABI only)

constexpr int kPipeSets = 4;   // workspace sets of ONE pipeline: packed, walked, being finalized, and one that is re-zeroed
constexpr int kPipes = 2;      // pipeline instances (twin: volumes are dealt alternately onto both); instance p owns sets p * kPipeSets ...
constexpr int kAllPipeSets = kPipes * kPipeSets;   // (the lanes' sets lie behind them)
inline bool pipe_set(int set) { return set >= 0 && set < kAllPipeSets; }
inline int next_pipe_set(int set) { return set - set % kPipeSets + (set + 1) % kPipeSets; }   // the next set of the same instance
// automatic twin from this many voxels (512^3): the smallest size of the sweep 128^3 ... 512^3 from which twin was faster in EVERY
// pair; the smaller sizes gained more on average (26 % at 128^3) but one pair of eight at 384^3 was slower
// (profiles/twin_pipeline_measurements.md section 3).  Never below 2^21: tests count the launches of the single pipeline on small volumes.
constexpr long long kTwinMinVoxels = 1LL << 27;

// The three word ranges of a volume that must be zero: accumulators + control words (before its WALKS), row flags and the four
// flag words (before its PACK).
enum { kZeroAcc = 0, kZeroRz = 1, kZeroFl = 2 };
constexpr size_t kFlagWords = 4;
struct ZeroWords {
  size_t w[3] = {0, 0, 0};
  size_t total() const { return w[0] + w[1] + w[2]; }
};
// What is known about the buffers of one workspace set.  A walk launch that carries a riding job re-zeroes what the set's last
// occupant used; the next occupant then needs no zero3_kernel if it needs no more than that and the buffers are still the same
// allocations.
struct SetZero {
  uintptr_t id[3] = {0, 0, 0};   // the buffers of the set's last occupant
  size_t rz_cap = 0;       // capacity of the row-flag allocation the record describes (a reallocation always grows it)
  size_t rz_used = 0;      // words the last occupant's pack may have written
  size_t rz_zero = 0;      // leading words known to be zero
  bool fl_zero = false;
};
struct PipePlanner {   // one per thread
  SetZero book[kAllPipeSets];
  unsigned long long seq[kPipes] = {0, 0};
  int pending[kPipes] = {-1, -1};   // set of the volume that is packed and not walked, or -1
  int walked[kPipes] = {-1, -1};    // set of the volume that is walked and not finalized, or -1
  unsigned long long twin_calls = 0;
};
inline bool pipe_busy(const PipePlanner &pl, int i) { return pl.pending[i] >= 0 || pl.walked[i] >= 0; }
inline bool pipe_busy(const PipePlanner &pl) { return pipe_busy(pl, 0) || pipe_busy(pl, 1); }

// ---- choosing: the instance and the set of a deferred call ------------------------------------------------------------------
struct PipeChoice {
  bool twin = false;
  int inst = 0, set = 0;
};
// twin_switch: PRAD_PIPE_TWIN (1, 0, or -1 = by the voxel count; voxels < 0: unknown)
inline PipeChoice pipe_choose(PipePlanner &pl, int twin_switch, long long voxels) {
  PipeChoice ch;
  ch.twin = twin_switch == 1 || (twin_switch < 0 && voxels >= kTwinMinVoxels);
  if (ch.twin) ch.inst = (int)(pl.twin_calls++ % (unsigned)kPipes);
  // Four workspace sets of the instance alternate.  The next one holds no volume in flight unless calls failed between their
  // choice and their step (each took a set): such a set is passed over, its volume is still to be walked or finished.
  do ch.set = ch.inst * kPipeSets + (int)(pl.seq[ch.inst]++ % (unsigned)kPipeSets);
  while (ch.set == pl.pending[ch.inst] || ch.set == pl.walked[ch.inst]);
  return ch;
}

// ---- preparing: what of a volume's three ranges zero3_kernel (or a riding job) still has to zero --------------------------------
// `id` / `words`: the volume's buffers and how much of each it uses (no row flags: id 0, 0 words); rz_cap: the capacity of the
// row-flag allocation.  What an earlier walk launch re-zeroed is not asked for again -- with fin_ride, and only while the buffer is
// the allocation the book describes.  The set is the volume's afterwards: its pack dirties the row flags and the flag words.
inline ZeroWords pipe_prepare(PipePlanner &pl, int set, const uintptr_t id[3], const size_t words[3], size_t rz_cap, bool fin_ride) {
  ZeroWords z;
  for (int r = 0; r < 3; r++) z.w[r] = words[r];
  SetZero &S = pl.book[set];
  if (fin_ride) {
    if (S.id[kZeroRz] == id[kZeroRz] && S.rz_cap == rz_cap && words[kZeroRz] <= S.rz_zero) z.w[kZeroRz] = 0;
    if (S.id[kZeroFl] == id[kZeroFl] && S.fl_zero) z.w[kZeroFl] = 0;
  }
  for (int r = 0; r < 3; r++) S.id[r] = id[r];
  S.rz_cap = rz_cap;
  S.rz_used = words[kZeroRz];
  S.rz_zero = 0;
  S.fl_zero = false;
  return z;
}

// ---- stepping: the launches of one deferred call, or of a flush ---------------------------------------------------------------
enum { kLaunchZero3 = 0, kLaunchFinalize = 1, kLaunchWalk = 2, kLaunchPack = 3 };
struct ZeroRange {
  int set = -1;
  size_t words = 0;
};
struct PipeLaunch {
  int kind = kLaunchZero3;
  int walk = -1;     // walk: the set of the volume it walks
  int pack = -1;     // walk: the set of the volume whose pack rides; pack: the set it packs
  int fin = -1;      // finalize: the set it finishes; walk: the set whose finalize rides
  bool job = false;  // walk: the launch may carry a riding job (FinJob), empty or not
  ZeroRange z[3];    // by kind of range (kZeroAcc ...).  zero3: what it zeroes; walk: what the riding job zeroes
};
struct PipeStep {
  int n = 0;
  PipeLaunch l[6];   // in launch order.  A finalize launch in front of the walk launch finishes the WALKED volume, one behind it
                     // the PENDING one.
  bool keep = false; // the walked volume's finalize is left to the next walk launch: the pending volume becomes `walked`
  PipeLaunch &add(int kind) {
    l[n] = PipeLaunch();
    l[n].kind = kind;
    return l[n++];
  }
};
struct StepInput {
  int inst = 0;
  int new_set = -1;        // the set of the call's volume (prepared: pipe_prepare); -1: a flush, nothing is packed
  ZeroWords need;          // what pipe_prepare left to zero for it
  // the conditions that depend on the volumes' plans and on the stream (prad_pipeline.h computes them)
  bool host_ok = false;          // fin_host_ok: the pending volume's walk launch, on this stream, can carry a riding job
  bool walked_can_ride = false;  // fin_can_ride of the walked volume
  bool pending_can_stay = false; // PRAD_FIN_RIDE is on and fin_can_ride of the pending volume
  bool pack_inline = false;      // the new volume's pack rides in the walk launch (pack_inline_ok, same kind of table)
};

// INVARIANT: no launch contains a word that one workgroup zeroes and any other workgroup of that launch reads or writes.
// It holds by construction, HERE: a riding range is named only after its SET has been compared with the sets of the three volumes
// the launch works on -- W (walked by it), P (packed by it), F (finished by it) -- and lies inside the instance; everything
// earlier is ordered by the stream.  tests/test_pipe_plan.py checks every record of many scripts against it.
inline PipeStep pipe_step(PipePlanner &pl, const StepInput &in) {
  PipeStep st;
  const int i = in.inst, base = i * kPipeSets;
  const int W = pl.pending[i], P = in.new_set, F = pl.walked[i];
  ZeroWords first = in.need;   // zero3_kernel in front of the launch: all of it unless the walk launch carries a job
  if (P < 0) first = ZeroWords();
  auto zero3 = [&](const ZeroWords &z) {
    if (z.total() == 0) return;
    PipeLaunch &L = st.add(kLaunchZero3);
    for (int r = 0; r < 3; r++)
      if (z.w[r] > 0) L.z[r].set = P, L.z[r].words = z.w[r];
  };
  if (W < 0) {   // nothing to walk: the first call of a run (a walked volume without a pending one: only after a failed call)
    if (F >= 0) st.add(kLaunchFinalize).fin = F;
    zero3(first);
  } else {
    // the walk launch zeroes the accumulators of the new volume itself if it carries a job; what the pack needs zeroed goes first
    const bool ride = P >= 0 && in.host_ok && in.need.total() < ((size_t)1 << 30);
    if (ride) first.w[kZeroAcc] = 0;
    zero3(first);
    // the finalize of the volume walked BEFORE rides in this launch if it can, else it is launched first
    const bool rides = in.host_ok && F >= 0 && in.walked_can_ride && F != W && F != P;
    if (F >= 0 && !rides) st.add(kLaunchFinalize).fin = F;
    PipeLaunch walk;
    walk.kind = kLaunchWalk;
    walk.walk = W;
    walk.pack = in.pack_inline ? P : -1;
    walk.fin = rides ? F : -1;
    walk.job = in.host_ok;
    const bool mine = P >= base && P < base + kPipeSets;
    if (in.host_ok && mine) {
      if (ride && in.need.w[kZeroAcc] > 0 && P != W && P != walk.fin) {
        walk.z[kZeroAcc].set = P;
        walk.z[kZeroAcc].words = in.need.w[kZeroAcc];
      }
      // the row flags and the flag words of the NEXT set, as its last occupant left them
      const int t = next_pipe_set(P);
      SetZero &S = pl.book[t];
      if (t != W && t != walk.fin && t != P) {
        if (S.rz_zero < S.rz_used && S.id[kZeroRz]) {
          walk.z[kZeroRz].set = t;
          walk.z[kZeroRz].words = S.rz_used;
          S.rz_zero = S.rz_used;
        }
        if (S.id[kZeroFl] && !S.fl_zero) {
          walk.z[kZeroFl].set = t;
          walk.z[kZeroFl].words = kFlagWords;
          S.fl_zero = true;
        }
      }
    }
    if (ride && in.need.w[kZeroAcc] > 0 && walk.z[kZeroAcc].set < 0) {   // (the job did not take the accumulators: their set is one the launch works on)
      ZeroWords acc;
      acc.w[kZeroAcc] = in.need.w[kZeroAcc];
      zero3(acc);
    }
    st.l[st.n++] = walk;
    st.keep = P >= 0 && in.pending_can_stay;
    if (!st.keep) st.add(kLaunchFinalize).fin = W;
  }
  if (P >= 0 && !(W >= 0 && in.pack_inline)) st.add(kLaunchPack).pack = P;
  pl.walked[i] = st.keep ? W : -1;
  pl.pending[i] = P;
  return st;
}

// ---- forgetting -------------------------------------------------------------------------------------------------------------------
// the workspace went away (prad_release_workspace) or the device changed: nothing is known to be zero, nothing is in flight
inline void pipe_forget(PipePlanner &pl) {
  for (int s = 0; s < kAllPipeSets; s++) pl.book[s] = SetZero();
  for (int i = 0; i < kPipes; i++) pl.pending[i] = pl.walked[i] = -1;
}
// a step of instance i could not be enqueued: what its record promised did not happen
inline void pipe_abandon(PipePlanner &pl, int i) {
  for (int s = i * kPipeSets; s < (i + 1) * kPipeSets; s++) pl.book[s] = SetZero();
  pl.pending[i] = pl.walked[i] = -1;
}

// ---- replay (prad_debug_pipe_plan; the layouts of an event and of a record: include/pyradiomics_amd.h) -----------------------------
constexpr int kPipeEventInts = 14, kPipeRecordInts = 13;
// Runs `n` events through a fresh planner as the executor runs calls through the thread's, and appends one record per launch.
inline void pipe_replay(const long long *events, int n, std::vector<int> &out) {
  struct Vol {   // what the executor's conditions read of a volume
    bool fused = false, can_ride = false, host_plan_ok = false;
  };
  PipePlanner pl;
  Vol pending[kPipes], walked[kPipes];
  long long stream[kPipes] = {0, 0};
  bool has_stream[kPipes] = {false, false};
  auto emit = [&](int ev, int inst, const PipeStep &st) {
    for (int k = 0; k < st.n; k++) {
      const PipeLaunch &L = st.l[k];
      const int r[kPipeRecordInts] = {ev, L.kind, inst, L.walk, L.pack, L.fin, L.job ? 1 : 0, L.z[0].set, (int)L.z[0].words,
                                      L.z[1].set, (int)L.z[1].words, L.z[2].set, (int)L.z[2].words};
      out.insert(out.end(), r, r + kPipeRecordInts);
    }
  };
  auto step = [&](int ev, StepInput in, bool fin_ride, bool same_stream) {
    const int i = in.inst;
    const bool have = pl.pending[i] >= 0;
    in.host_ok = have && fin_ride && same_stream && pending[i].fused && pending[i].host_plan_ok;
    in.walked_can_ride = pl.walked[i] >= 0 && walked[i].can_ride;
    in.pending_can_stay = have && fin_ride && pending[i].can_ride;
    const PipeStep st = pipe_step(pl, in);
    if (st.keep) walked[i] = pending[i];
    emit(ev, i, st);
  };
  auto flush = [&](int ev, int i, bool fin_ride) {
    if (!pipe_busy(pl, i)) return;
    StepInput in;
    in.inst = i;
    step(ev, in, fin_ride, true);
  };
  for (int ev = 0; ev < n; ev++) {
    const long long *e = events + (size_t)ev * kPipeEventInts;
    const int type = (int)e[0];
    const bool fin_ride = e[9] != 0;
    if (type != 1 && type != 3) {   // 0: a flush (join, status, mark); 2: the workspace is released
      for (int i = 0; i < kPipes; i++) flush(ev, i, fin_ride);
      if (type == 2) pipe_forget(pl);
      continue;
    }
    const int kind = (int)e[4];   // 0 fused table, 1 two tables, 2 a volume the pipeline does not take
    const PipeChoice ch = pipe_choose(pl, (int)e[5], e[1]);
    const int i = ch.inst;
    if (!ch.twin) flush(ev, 1, fin_ride);   // (instance 1 holds volumes of twin calls only)
    if (e[13] != 0) flush(ev, 1 - i, fin_ride);   // an output buffer that the other instance still writes
    if (type == 3) continue;   // a call that fails behind the choice of its set (arguments no call accepts): nothing else happens
    if (kind == 2) {
      for (int k = 0; k < kPipes; k++) flush(ev, k, fin_ride);
      continue;
    }
    const long long s = ch.twin ? -1 - i : e[6];   // (a twin call runs on the instance's internal stream)
    const size_t rz_words = kind == 0 ? (size_t)((e[2] + 3) / 4) : 0;   // (only the fused-table walk has row flags)
    const uintptr_t id[3] = {(uintptr_t)(0xA000 + ch.set), rz_words ? (uintptr_t)e[7] : 0, (uintptr_t)(0xF000 + ch.set)};
    const size_t words[3] = {(size_t)e[3], rz_words, kFlagWords};
    StepInput in;
    in.inst = i;
    in.new_set = ch.set;
    in.need = pipe_prepare(pl, ch.set, id, words, rz_words ? (size_t)e[8] : 0, fin_ride);
    in.pack_inline = pl.pending[i] >= 0 && e[12] != 0 && pending[i].fused == (kind == 0);
    step(ev, in, fin_ride, has_stream[i] && stream[i] == s);
    pending[i].fused = kind == 0;
    pending[i].can_ride = e[10] != 0;
    pending[i].host_plan_ok = e[11] != 0;
    stream[i] = s;
    has_stream[i] = true;
  }
}

#pragma GCC visibility pop
}  // namespace prad
