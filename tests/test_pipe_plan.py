"""The planner of the deferred GLCM + GLRLM pipeline (csrc/prad_pipe_plan.h) against a model of the workspace.  Scripts of events
(deferred calls, flushes, workspace releases) are replayed through a fresh planner by prad_debug_pipe_plan
(include/pyradiomics_amd.h has the layouts); every launch record is then held to the model.  Host only: no device call is made.

The model.  Per workspace set three regions: `acc` (accumulators + control words), `rz` (row flags), `fl` (the four flag words);
per region the leading words known to be zero and the extent that may be dirty.  What a job touches, read off the kernels
(kernels_sweepfw.h sweep_fw_kernel, PackWave, FinJob; kernels_sweepfw2.h; kernels_sweep.h finalize_volume_kernel):

    walk of set W       reads rz and fl (flags[0], flags[3]) of W, adds into acc of W (matrices, multi words, work counters)
    pack into set P     writes rz and fl (flags[0], flags[3]) of P
    finalize of set F   reads acc and fl of F, writes into the control words (and the run table) of acc of F

Checked on every record of every script:
  1. INVARIANT      no riding zero range names a region that the same launch's walk, pack or finalize touches; a zero3_kernel
                    launch does nothing else; no launch names a set outside its own instance.
  2. SUFFICIENCY    when a volume is packed, its rz words and fl are zero; when it is walked, its acc words are zero -- zeroed by
                    a STRICTLY EARLIER launch of the same instance and not dirtied since, in a buffer of the same id and capacity.
                    And across launches: nothing in flight is zeroed (rz between pack and walk, fl and acc up to the finalize),
                    and a set is packed only after its last occupant was finalized.
  3. ECONOMY        a run of six same-shaped fused-table volumes plans at most two stand-alone finalize launches; from the first
                    call whose set a riding job re-zeroed, no zero3_kernel; with PRAD_FIN_RIDE=0 six of each.
  4. DRAINS         a flush, a workspace release and a call the pipeline does not take leave nothing pending or walked in either
                    instance; a call that is not twin leaves instance 1 empty.
                    A two-table call and a change of stream do NOT empty the instance in this pipeline and never did: the new
                    volume is pending behind them, and the volume walked by that step may stay walked.  What holds, and is
                    asserted: a walk launch on another stream than its volume's pack, or of a two-table volume, carries no
                    riding job; the volume walked before it is finished by a launch of its own first; a two-table volume is
                    finished behind its own walk launch."""
import ctypes as C
import random

import numpy as np
import pytest

EVENT_INTS, RECORD_INTS = 14, 13
ZERO3, FINALIZE, WALK, PACK = 0, 1, 2, 3
ACC, RZ, FL = 0, 1, 2
FUSED, TWO_TABLE, NOT_PIPELINE = 0, 1, 2
SETS, PIPES = 4, 2
TWIN_MIN_VOXELS = 1 << 27
SHAPE = (9, 40, 130)


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


# ---- events -----------------------------------------------------------------------------------------------------------------------
def acc_words(shape, Ng=32, Na=13):
    """accumulators + control words of a GLCM + GLRLM volume (csrc/prad_api.hip vol_prepare); the control words: any constant"""
    return Na * Ng * Ng + Na * Ng * max(shape) + 2000


def call(shape=SHAPE, Ng=32, kind=None, twin=-1, stream=0, fin_ride=1, can_ride=None, host_plan_ok=None, inline=1, overlap=0,
         voxels=None, acc=None):
    kind = (FUSED if Ng <= 44 else TWO_TABLE) if kind is None else kind
    return dict(type=1, voxels=int(np.prod(shape)) if voxels is None else voxels, rows=shape[0] * shape[1],
                acc=acc_words(shape, Ng) if acc is None else acc, kind=kind, twin=twin, stream=stream, fin_ride=fin_ride,
                can_ride=int(kind == FUSED) if can_ride is None else can_ride,
                host_plan_ok=int(kind == FUSED) if host_plan_ok is None else host_plan_ok, inline=inline, overlap=overlap)


def flush(fin_ride=1):
    return dict(type=0, fin_ride=fin_ride)


def release(fin_ride=1):
    return dict(type=2, fin_ride=fin_ride)


def failed(**kw):
    """a deferred call that fails behind the choice of its set: it takes a set and launches nothing of its own"""
    return dict(call(**kw), type=3)


class Buffers:
    """the row-flag buffer of every set as the library's workspace would hold it: it grows when a volume needs more (a new id, a
    larger capacity), and a test may have it allocated anew (a new id, the same capacity)"""

    def __init__(self):
        self.next_id = 1000
        self.buf = {}

    def get(self, s, rows, renew=False):
        need = rows + 64
        ident, cap = self.buf.get(s, (0, 0))
        if cap < need:
            cap = need + need // 8 + 256
            renew = True
        if renew:
            self.next_id += 1
            ident = self.next_id
        self.buf[s] = (ident, cap)
        return ident, cap

    def drop(self):
        self.buf = {}


def replay(lib, raw):
    out = np.zeros(RECORD_INTS * 6 * 3 * max(1, len(raw)), dtype=np.int32)
    got = lib.prad_debug_pipe_plan(raw.ctypes.data_as(C.POINTER(C.c_longlong)), len(raw), out.ctypes.data_as(C.POINTER(C.c_int)),
                                   len(out))
    assert got >= 0 and got % RECORD_INTS == 0, got
    per_event = [[] for _ in raw]
    for r in out[:got].reshape(-1, RECORD_INTS).tolist():
        per_event[r[0]].append(r)
    return per_event


def plan(lib, events):
    """-> (per event: its launch records, the events with their row-flag buffers filled in).  Which set a call gets does not
    depend on its buffers: a first replay with one buffer for all tells the sets (the model has its own opinion on them, below),
    the test then gives every set's buffer the id and the capacity the workspace would, and replays again."""
    raw = np.zeros((len(events), EVENT_INTS), dtype=np.int64)
    for n, e in enumerate(events):
        raw[n, 0], raw[n, 9] = e["type"], e["fin_ride"]
        if e["type"] in (1, 3):
            raw[n, 1:9] = [e["voxels"], e["rows"], e["acc"], e["kind"], e["twin"], e["stream"], 7, 1 << 40]
            raw[n, 10:14] = [e["can_ride"], e["host_plan_ok"], e["inline"], e["overlap"]]
    bufs = Buffers()
    for e, records in zip(events, replay(lib, raw)):
        if e["type"] == 2:
            bufs.drop()
        if e["type"] != 1 or e["kind"] == NOT_PIPELINE:
            continue
        (e["set"],) = [r[4] for r in records if r[4] >= 0]
        e["rz_words"] = (e["rows"] + 3) // 4 if e["kind"] == FUSED else 0
        e["rz_id"], e["rz_cap"] = bufs.get(e["set"], e["rows"], e.get("renew", False)) if e["kind"] == FUSED else (0, 0)
    for n, e in enumerate(events):
        if e["type"] == 1 and e["kind"] != NOT_PIPELINE:
            raw[n, 7:9] = [e["rz_id"], e["rz_cap"]]
    return replay(lib, raw), events


def test_record_buffer_too_small(lib):
    raw = np.zeros((2, EVENT_INTS), dtype=np.int64)
    raw[0, :13] = [1, 1000, 10, 500, FUSED, 0, 0, 77, 512, 1, 1, 1, 1]
    raw[1, 9] = 1      # a flush
    out = np.zeros(4 * RECORD_INTS, dtype=np.int32)
    args = (raw.ctypes.data_as(C.POINTER(C.c_longlong)), 2, out.ctypes.data_as(C.POINTER(C.c_int)))
    assert lib.prad_debug_pipe_plan(*args, 4 * RECORD_INTS) == 4 * RECORD_INTS      # zero3, pack; walk, finalize
    assert lib.prad_debug_pipe_plan(*args, 4 * RECORD_INTS - 1) == -4 * RECORD_INTS


# ---- the model --------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self):
        self.forget()
        self.launch = 0
        self.seq, self.twin_calls = [0] * PIPES, 0
        self.stats = dict(zero3=0, finalize=0, walk=0, pack=0, rode=0)

    def forget(self):
        self.zero = [[0, 0, 0] for _ in range(SETS * PIPES)]      # leading words known to be zero
        self.dirty = [[0, 0, 0] for _ in range(SETS * PIPES)]     # extent that may have been written since
        self.rz_buf = [(0, 0)] * (SETS * PIPES)
        self.vol = [None] * (SETS * PIPES)                        # the set's occupant: the call event + its stage
        self.rezeroed = set()                                     # sets a riding job has re-zeroed (row flags or flag words)

    def busy(self, inst=None):
        return [s for s in range(SETS * PIPES) if self.vol[s] is not None and (inst is None or s // SETS == inst)]

    def _dirty(self, s, r, words):
        self.zero[s][r] = 0
        self.dirty[s][r] = max(self.dirty[s][r], words)

    def _zeroed(self, s, r, words):
        self.zero[s][r] = max(self.zero[s][r], words)
        if words >= self.dirty[s][r]:
            self.dirty[s][r] = 0

    def choose(self, e):
        """CHOOSING: twin by the switch or the voxel count; twin calls alternate between the instances; the sets of an instance
        alternate, and one that still holds a volume (calls failed in between) is passed over"""
        e["twin_call"] = e["twin"] == 1 or (e["twin"] < 0 and e["voxels"] >= TWIN_MIN_VOXELS)
        e["inst"] = 0
        if e["twin_call"]:
            e["inst"] = self.twin_calls % PIPES
            self.twin_calls += 1
        while True:
            s = e["inst"] * SETS + self.seq[e["inst"]] % SETS
            self.seq[e["inst"]] += 1
            if self.vol[s] is None:
                return s

    def event(self, n, e, records):
        ctx = "event %d %r" % (n, {k: v for k, v in e.items() if k != "type"})
        new = e["type"] == 1 and e["kind"] != NOT_PIPELINE
        chosen = self.choose(e) if e["type"] in (1, 3) else None
        if new:
            P = e["set"]
            packs = [r for r in records if r[4] >= 0]
            assert len(packs) == 1 and packs[0][4] == P == chosen and packs[0][2] == e["inst"], (ctx, chosen, records)
            if e["kind"] == FUSED and self.rz_buf[P] != (e["rz_id"], e["rz_cap"]):      # another allocation: contents unknown
                self.zero[P][RZ], self.dirty[P][RZ] = 0, e["rz_cap"] // 4
            if e["kind"] == FUSED:
                self.rz_buf[P] = (e["rz_id"], e["rz_cap"])
            self.zero[P][ACC] = 0      # (the accumulator buffer may have grown: nothing of it is taken for zero)
        else:
            assert all(r[4] < 0 for r in records), (ctx, records)
        for r in records:
            self.record(ctx, e, r)
        # ---- 4. drains
        if e["type"] == 3:
            assert e["twin_call"] or not self.busy(1), (ctx, "instance 1 holds volumes of twin calls only")
        elif not new:
            assert not self.busy(), (ctx, "left in flight", self.busy())
        else:
            if not e["twin_call"]:
                assert not self.busy(1), (ctx, "instance 1 holds volumes of twin calls only")
            mine = self.busy(e["inst"])
            walked = [s for s in mine if self.vol[s]["stage"] == "walked"]
            assert [s for s in mine if self.vol[s]["stage"] == "packed"] == [e["set"]] and len(walked) <= 1, (ctx, mine)
            for s in walked:      # only a volume whose finalize can ride waits for the next walk launch
                w = self.vol[s]["call"]
                assert w["kind"] == FUSED and w["can_ride"] and e["fin_ride"], (ctx, w)
        if e["type"] == 2:
            self.forget()

    def record(self, ctx, e, r):
        ev, kind, inst, W, P, F, job = r[:7]
        ranges = [(r[7 + 2 * k], k, r[8 + 2 * k]) for k in range(3) if r[7 + 2 * k] >= 0]
        ctx = (ctx, "launch", r)
        self.launch += 1
        self.stats[("zero3", "finalize", "walk", "pack")[kind]] += 1
        # ---- 1. invariant
        for s in [W, P, F] + [z[0] for z in ranges]:
            assert s < 0 or s // SETS == inst, (ctx, "a set of the other instance")
        touched = set()
        if W >= 0:
            touched |= {(W, RZ), (W, FL), (W, ACC)}
        if P >= 0:
            touched |= {(P, RZ), (P, FL)}
        if F >= 0:
            touched |= {(F, ACC), (F, FL)}
        assert kind in (ZERO3, WALK) or not ranges, ctx
        assert kind != ZERO3 or (ranges and not touched), ctx
        assert kind == WALK or (W < 0 and job == 0), ctx
        assert kind != WALK or W >= 0, ctx
        assert kind != FINALIZE or (F >= 0 and P < 0), ctx
        assert kind != PACK or (P >= 0 and F < 0), ctx
        for s, k, words in ranges:
            assert words > 0 and (s, k) not in touched, (ctx, "zeroes what the launch works on", (s, k))
        if ranges and kind == WALK:
            assert job == 1, ctx
        if F >= 0 and kind == WALK:
            assert job == 1, ctx
            self.stats["rode"] += 1
        # ---- 2. sufficiency, from what strictly earlier launches left
        if P >= 0:
            assert self.vol[P] is None, (ctx, "the set's last occupant is not finalized", self.vol[P])
            assert P == e["set"], ctx
            assert self.zero[P][RZ] >= e["rz_words"], (ctx, "row flags not zero", self.zero[P][RZ], e["rz_words"])
            assert self.zero[P][FL] >= 4, (ctx, "flag words not zero")
        if W >= 0:
            v = self.vol[W]
            assert v is not None and v["stage"] == "packed", (ctx, v)
            assert self.zero[W][ACC] >= v["call"]["acc"], (ctx, "accumulators not zero", self.zero[W][ACC], v["call"]["acc"])
            if job:      # (4.) only a fused-table launch on the stream of its volume's pack carries a job
                assert v["call"]["kind"] == FUSED and v["call"]["host_plan_ok"] and e["fin_ride"], ctx
                step = e["type"] == 1 and e["kind"] != NOT_PIPELINE and inst == e["inst"]      # (else a flush: on the pack's stream)
                assert not step or v["stream"] == self.stream_of(e), (ctx, "a job across streams")
        if F >= 0:
            v = self.vol[F]
            assert v is not None and v["stage"] == ("packed" if F == W else "walked"), (ctx, v)
            if kind == WALK:
                assert F != W and v["call"]["can_ride"], ctx
        for s, k, words in ranges:      # nothing in flight is zeroed
            v = self.vol[s]
            if v is not None:
                assert k == ACC and v["stage"] == "packed", (ctx, "zeroes a range of a volume in flight", (s, k), v)
        # ---- the launch's effects
        if W >= 0:
            self._dirty(W, ACC, self.vol[W]["call"]["acc"])
            self.vol[W]["stage"] = "walked"
        if P >= 0:
            if e["rz_words"]:
                self._dirty(P, RZ, e["rz_words"])
            self._dirty(P, FL, 4)
        if F >= 0:
            self.vol[F] = None
        if P >= 0:
            self.vol[P] = dict(call=e, stage="packed", stream=self.stream_of(e))
        for s, k, words in ranges:
            self._zeroed(s, k, words)
            if kind == WALK and k != ACC:
                self.rezeroed.add(s)

    @staticmethod
    def stream_of(e):
        return ("twin", e["inst"]) if e["twin_call"] else ("user", e["stream"])


def check(lib, events):
    """the script through the replay and the model -> (the model, launch records per event)"""
    per_event, events = plan(lib, events)
    m = Model()
    for n, (e, records) in enumerate(zip(events, per_event)):
        m.event(n, e, records)
    return m, per_event


def kinds(records, kind):
    return sum(1 for rs in records for r in rs if r[1] == kind)


# ---- the sequences of test_gpu_fin_ride.py ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 65), (9, 40, 130), (12, 20, 257), (20, 24, 512)])
def test_runs_of_one_shape(lib, shape):
    for n in range(1, 7):
        for ride in (1, 0):
            m, recs = check(lib, [call(shape, fin_ride=ride) for _ in range(n)] + [flush(ride)])
            assert m.stats["walk"] == n and m.stats["pack"] == 1
            if not ride:      # 3. every volume its own zero3_kernel and its own stand-alone finalize
                assert m.stats["zero3"] == n and m.stats["finalize"] == n and m.stats["rode"] == 0
    m, recs = check(lib, [call(shape) for _ in range(6)] + [flush()])
    assert m.stats["finalize"] <= 2 and m.stats["finalize"] + m.stats["rode"] == 6      # 3. the bound of the device test


def test_no_zero3_once_a_riding_job_has_rezeroed_the_set(lib):
    for twin in (0, 1):
        events = [call(SHAPE, twin=twin) for _ in range(24)]
        per_event, events = plan(lib, events)
        m, steady = Model(), None
        for n, (e, records) in enumerate(zip(events, per_event)):
            if steady is None and e["set"] in m.rezeroed:
                steady = n
            m.event(n, e, records)
            if steady is not None:
                assert not [r for r in records if r[1] in (ZERO3, FINALIZE, PACK)], (n, records)      # ONE launch per step
        assert steady is not None and steady <= (5 if not twin else 10)


def test_changing_shapes(lib):
    shapes = [(24, 30, 512), (20, 26, 256), (18, 22, 300), (30, 30, 64), (24, 30, 512)]
    for seq in (shapes, shapes[::-1]):
        for ride in (1, 0):
            check(lib, [call(s, fin_ride=ride) for s in seq] + [flush(ride)])


@pytest.mark.parametrize("first", ["large", "small"])
def test_zero_extents(lib, first):
    large, small = [call((9, 40, 130)) for _ in range(5)], [call((2, 2, 65)) for _ in range(5)]
    a, b = (large, small) if first == "large" else (small, large)
    for seq in (a + b, a[:4] + b[:1] + a[4:] + b[1:]):
        for ride in (1, 0):
            m, _ = check(lib, [dict(e, fin_ride=ride) for e in seq] + [flush(ride)])
            assert m.stats["walk"] == 10


def test_fused_and_two_table_alternating(lib):
    specs = [((12, 20, 257), 32), ((12, 20, 257), 64), ((9, 40, 130), 32), ((9, 40, 130), 64), ((20, 24, 512), 32), ((16, 16, 128), 48)]
    vols = [call(s, Ng) for s, Ng in specs]
    for seq in (vols, vols + vols[:1] + vols[2:3] + vols[4:] + vols[:2]):
        for ride in (1, 0):
            m, recs = check(lib, [dict(e, fin_ride=ride) for e in seq] + [flush(ride)])
            # a two-table volume is finished behind its own walk launch, and no job rides in that launch
            for e, rs in zip(seq[:-1], recs[1:]):
                if e["kind"] == TWO_TABLE:
                    walk = [r for r in rs if r[1] == WALK]
                    assert len(walk) == 1 and walk[0][6] == 0 and [r[5] for r in rs if r[1] == FINALIZE][-1] == walk[0][3]


@pytest.mark.parametrize("after", [0, 1, 2, 4])
def test_mark_in_the_middle(lib, after):
    events = [call(SHAPE) for _ in range(6)]
    events.insert(after + 1, flush())
    m, recs = check(lib, events + [flush()])
    assert m.stats["walk"] == 6 and m.stats["pack"] == 2


@pytest.mark.parametrize("switch", ["can_ride", "host_plan_ok"])
def test_route_stands_aside(lib, switch):
    """PRAD_FW_XROLE=0 / PRAD_FINALIZE_ONE=0 (no finalize can ride), a plan whose launch carries no job: 6 of 6 stand alone"""
    m, _ = check(lib, [call((12, 20, 257), **{switch: 0}) for _ in range(6)] + [flush()])
    assert m.stats["finalize"] == 6 and m.stats["rode"] == 0
    assert m.stats["zero3"] == (6 if switch == "host_plan_ok" else 4)      # (a job without a finalize still zeroes)


# ---- twin, streams, buffers ---------------------------------------------------------------------------------------------------------
def test_twin_on_off_and_switching(lib):
    for ride in (1, 0):
        m, _ = check(lib, [call(SHAPE, twin=1, fin_ride=ride) for _ in range(11)] + [flush(ride)])
        assert m.stats["walk"] == 11 and m.stats["pack"] == 2
        check(lib, [call(SHAPE, twin=t, fin_ride=ride) for t in (0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 1, -1, -1)] + [flush(ride)])
    big = dict(shape=SHAPE, voxels=TWIN_MIN_VOXELS)
    _, events = plan(lib, [call(**big), call(**big), call(SHAPE, voxels=TWIN_MIN_VOXELS - 1), call(**big)])
    assert [e["set"] for e in events] == [0, 4, 1, 2]      # automatic twin from 2^27 voxels: instances 0, 1; not twin; 0
    check(lib, [call(**big) for _ in range(9)] + [flush()])


def test_alternating_streams(lib):
    m, recs = check(lib, [call(SHAPE, stream=n % 2) for n in range(10)] + [flush()])
    # no job crosses from one stream to the other: every call's walk launch goes without (the flush, on the stream of the last
    # call, may carry the finalize of the volume that call walked there)
    assert not [r for rs in recs[:10] for r in rs if r[1] == WALK and r[6]]
    assert m.stats["finalize"] + m.stats["rode"] == 10 and m.stats["rode"] <= 1
    m, recs = check(lib, [call(SHAPE, stream=n // 5) for n in range(10)] + [flush()])
    assert m.stats["finalize"] <= 4


def test_growing_and_reallocated_row_flags(lib):
    grow = [call((3 + 2 * n, 40, 130)) for n in range(12)]      # every volume has more rows than its set's last occupant
    m, recs = check(lib, grow + [flush()])
    assert all(any(r[1] == ZERO3 and r[9] >= 0 for r in rs) for rs in recs[:12])      # ... so zero3_kernel zeroes its row flags
    events = [call(SHAPE) for _ in range(16)]
    events[9]["renew"] = True      # the same capacity at a new address
    m, recs = check(lib, events + [flush()])
    assert [n for n, rs in enumerate(recs) if any(r[1] == ZERO3 for r in rs)] == [0, 1, 2, 3, 9]
    check(lib, [call(SHAPE) for _ in range(6)] + [release()] + [call(SHAPE) for _ in range(6)] + [flush()])


def test_accumulators_beyond_the_jobs_word_count(lib):
    """2^30 words and more are zero3_kernel's; the riding job still re-zeroes the next set's row flags and flag words"""
    m, recs = check(lib, [call(SHAPE, acc=1 << 30) for _ in range(8)] + [flush()])
    assert m.stats["zero3"] == 8 and m.stats["rode"] == 7 and m.stats["finalize"] == 1      # (the last volume: behind the flush)
    assert all(r[7] < 0 for rs in recs for r in rs if r[1] == WALK)


def test_calls_that_fail_take_sets(lib):
    """a set that still holds a volume is passed over; the riding job never zeroes the row flags of the volume its launch walks
    (two sets taken by failed calls put the new volume's NEXT set onto the walked one)"""
    for nfail in range(0, 9):
        for can_ride in (1, 0):
            for at in (1, 2, 3, 5):
                events = [call(SHAPE, can_ride=can_ride) for _ in range(8)]
                events[at:at] = [failed() for _ in range(nfail)]
                check(lib, events + [flush()])
    m, recs = check(lib, [call(SHAPE, can_ride=0), call(SHAPE, can_ride=0), failed(), failed(), call(SHAPE), flush()])
    assert [e for e in recs[4] if e[1] == WALK][0][3:5] == [1, 0]      # walks set 1, packs set 0, whose next set is set 1


# ---- random scripts -----------------------------------------------------------------------------------------------------------------
def random_script(rng):
    shapes = [(2, 2, 65), (9, 40, 130), (12, 20, 257), (20, 24, 512), (64, 64, 64), (3, 5, 1024)]
    events, twin, stream, ride = [], rng.choice([-1, 0, 1]), 0, 1
    shape = rng.choice(shapes)
    for _ in range(rng.randint(1, 40)):
        if rng.random() < 0.15:
            twin = rng.choice([-1, 0, 1])
        if rng.random() < 0.1:
            stream = 1 - stream
        if rng.random() < 0.08:
            ride = 1 - ride
        if rng.random() < 0.3:
            shape = rng.choice(shapes)
        u = rng.random()
        if u < 0.06:
            events.append(flush(ride))
        elif u < 0.08:
            events.append(failed(shape=shape, twin=twin, stream=stream, fin_ride=ride))
        elif u < 0.10:
            events.append(release(ride))
        else:
            kind = FUSED if u < 0.8 else (TWO_TABLE if u < 0.95 else NOT_PIPELINE)
            e = call(shape, 32 if kind == FUSED else 64, kind=kind, twin=twin, stream=stream, fin_ride=ride,
                     inline=int(rng.random() < 0.8), overlap=int(rng.random() < 0.05),
                     voxels=TWIN_MIN_VOXELS if rng.random() < 0.1 else None, acc=(1 << 30) if rng.random() < 0.02 else None)
            if kind == FUSED:
                e["can_ride"], e["host_plan_ok"] = int(rng.random() < 0.9), int(rng.random() < 0.95)
                e["renew"] = rng.random() < 0.04
            events.append(e)
    return events + [flush(ride)]


def test_random_scripts(lib):
    rng = random.Random(20260)
    launches = rode = 0
    for _ in range(3000):
        m, _ = check(lib, random_script(rng))
        launches += m.launch
        rode += m.stats["rode"]
    assert launches > 50000 and rode > 5000      # (the scripts do reach the riding route)
