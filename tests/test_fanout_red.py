"""Fan-out that strips or adds RED per destination (srtp_fanout_device_red /
_host_red, k_fanout_red): each destination entry carries a 4-byte record (mode,
red_pt) for the one engine of the peer's send chain that moves the payload --
REDFilterTransformEngine.transform for a peer without RED,
REDTransformEngine.transform for a peer with it -- applied to the copy in front
of its other records and of the protect chain.

The expected result is the definition itself: entry j's bytes, length, status
and context state are those of the existing _pay rules for a source that
already held RED(source).  So red_ref.apply (the two Java methods restated)
makes each entry's source on the host, a dropped entry is flagged SKIP, and that
fan goes the way of the other fan-out tests: the setters, payload_ref,
abs_send_time_ref, then oracle.process / gcm_ref.process.  Every run asserts bit
equality of len, status, red_out, the bytes [off, off + len) of every OK entry,
the context state and, on the device route, every FILL byte outside the regions
rounded up to 16, the regions of skipped and dropped entries, and the source
segment.  The entries are tests/red_grids.py's, which a test without a GPU holds
to carry every result code."""
import numpy as np
import pytest

import red_grids as RG
from libjitsi_amd import _native as N
from test_fanout import FILL, RTP, SKIP, Peer, make_engine, seed, up16
from test_fanout_pay import PayFan, pay
from test_fanout_ast import stamp
from test_fanout_rewrite import rec

pytestmark = pytest.mark.gpu

CM, GCM = "AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM"
ROOM = {CM: 10, GCM: 16}
INVALID = N.STATUS_DROP_INVALID
ROUTES = [(r, p) for r in ("host", "device") for p in (CM, GCM)]
IDS = ["%s-%s" % (r, "cm" if p == CM else "gcm") for r, p in ROUTES]


class RedFan:
    """A grid of red_grids entries toward one peer: `f` holds the arrays the
    engine gets, `g` the fan of the sources as RED leaves them, which the
    references process."""

    def __init__(self, grid, peer, room, gaps=(16, 48), pass_red=True, which=0):
        self.grid, self.n, self.which = grid, len(grid), which
        caps = [e["cap"] if e["cap"] is not None else len(e["pkt"]) + 1 + room for e in grid]
        status = [e["status"] for e in grid]
        some = lambda k: any(e[k] is not None for e in grid)
        rws = [e["rw"] or rec() for e in grid] if some("rw") else None
        asts = [e["ast"] or stamp(0, 3, 0) for e in grid] if some("ast") else None
        pays = [e["pay"] or pay() for e in grid] if some("pay") else None
        exp = [RG.expect(e, room) if pass_red else (0, e["pkt"]) for e in grid]
        self.codes = np.array([r for r, _ in exp], np.int8)
        self.f = PayFan([e["pkt"] for e in grid], [(j, peer, caps[j], e["flags"]) for j, e in enumerate(grid)], rws, asts,
                        pays, gaps=gaps, src_status=status)
        self.g = PayFan([b for _, b in exp],
                        [(j, peer, caps[j], e["flags"] | (SKIP if exp[j][0] < 0 else 0)) for j, e in enumerate(grid)],
                        rws, asts, pays, gaps=gaps, src_status=status)
        assert np.array_equal(self.f.off, self.g.off) and self.f.seg_bytes == self.g.seg_bytes
        self.red = np.zeros(self.n, N.FANOUT_RED_DTYPE)
        self.red["mode"], self.red["red_pt"] = [e["red"][0] for e in grid], [e["red"][1] for e in grid]
        self.pass_red = pass_red

    def run_host(self, eng):
        f = self.f
        seg = np.full(f.seg_bytes, FILL, np.uint8)
        src = f.src_seg.copy()
        ln, st, ro = eng.fanout_host_red(f.tids, f.src_seg, f.src_off, f.src_len, f.src_cap, f.src_idx, seg, f.off,
                                         f.cap, f.src_status, f.flags if f.flags.any() else None, f.records(),
                                         f.stamps(), f.pays(), self.red if self.pass_red else None)
        assert np.array_equal(src, f.src_seg)
        return seg, ln, st, ro

    def run_device(self, eng, misalign=0):
        import torch
        f = self.f
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

        def records(arr, size, shift=0):
            if arr is None:
                return None
            raw = torch.zeros(size * f.n + 32, dtype=torch.uint8, device="cuda")
            raw[shift:shift + size * f.n].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()))
            return raw[shift:shift + size * f.n]
        src_seg = d(f.src_seg)
        seg = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
        ro = torch.full((f.n,), 77, dtype=torch.int8, device="cuda")
        args = [d(f.src_off), d(f.src_len), d(f.src_cap), d(f.src_idx), seg, d(f.off), ln, d(f.cap), st]
        rw, ast, py = records(f.records(), 16), records(f.stamps(), 8), records(f.pays(), 8)
        red = records(self.red if self.pass_red else None, 4, misalign)
        src_status = None if f.src_status is None else d(f.src_status)
        flags = d(f.flags) if f.flags.any() else None
        torch.cuda.synchronize()
        try:
            eng.fanout_device_red(d(f.tids), src_seg, *args, rw, ast, py, red, ro, src_status=src_status, flags=flags)
        finally:
            eng.sync(None)
            torch.cuda.synchronize()
            self.src_after = src_seg.cpu().numpy()
            self.seg_after = seg.cpu().numpy()
            self.ro_after = ro.cpu().numpy()
        return self.seg_after, ln.cpu().numpy().view(np.uint32), st.cpu().numpy(), self.ro_after

    def held(self, eng, route, **kw):
        f, g = self.f, self.g
        seg, ln, st, ro = self.run_host(eng) if route == "host" else self.run_device(eng, **kw)
        for j in range(self.n):
            print("entry %3d: red %s code %2d/%2d len %5d status %d" % (j, self.grid[j]["red"], ro[j], self.codes[j], ln[j],
                                                                        st[j]))
        assert ro.tolist() == (self.codes.tolist() if self.pass_red or route == "host" else [77] * self.n)
        _, ln_r, st_r = g.check(eng, (seg, ln, st), which=self.which)
        if route == "device":
            want = g.expand()[0]
            inside = np.zeros(f.seg_bytes, bool)
            for j in range(self.n):
                o, c = int(f.off[j]), up16(f.cap[j])
                if g.skipped(j)[0]:  # skipped, or dropped by RED: nothing is copied
                    assert st[j] == N.STATUS_SKIPPED and ln[j] == 0 and (seg[o:o + c] == FILL).all(), j
                    continue
                inside[o:o + c] = True
                if self.codes[j] == 2 and ln[j] > f.cap[j]:  # a wrap that does not fit: nothing is moved
                    assert st[j] == INVALID and (seg[o:o + c] == FILL).all(), j
                elif st[j] in (INVALID, N.STATUS_NOT_PROCESSED):  # the chain left the copy as it was expanded
                    k = max(g.copied(j), 0)
                    assert np.array_equal(seg[o:o + k], want[o:o + k]), j
                    assert (seg[o + up16(k):o + c] == FILL).all(), j
            assert (seg[~inside] == FILL).all()
            assert np.array_equal(self.src_after, f.src_seg)
        return seg, ln, st, ro


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


def all_codes(fan):
    assert set(fan.codes.tolist()) == {0, 1, 2, -1}


# ------------------------------------------------------------------ 1. boundaries
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_boundaries(eng, route, profile):
    """h over 12, 16, 20, 24, 28, 32 (CC 0..1, no extension, one word, three
    words), c at h and h + 1, around 32 and 48, around 1024 (lane 63's piece
    against lane 0's second) and around 2048 (the second trip), both modes; wrap
    into a destination of c + 1 bytes (fits) and of c (DROP_INVALID, nothing
    moved); strip of a 13-byte packet."""
    room = ROOM[profile]
    fan = RedFan(RG.boundaries(room), Peer([eng], RTP, profile, seed()), room)
    all_codes(fan)
    seg, ln, st, ro = fan.held(eng, route)
    fits = [j for j, e in enumerate(fan.grid) if e["cap"] == len(e["pkt"])]
    assert len(fits) == 4 and all(st[j] == INVALID and ro[j] == 2 and ln[j] == len(fan.grid[j]["pkt"]) + 1 for j in fits)
    ok = st == 0
    assert (ok & (ro == 1)).sum() > 40 and (ok & (ro == 2)).sum() > 60
    j13 = next(j for j, e in enumerate(fan.grid) if len(e["pkt"]) == 13 and e["red"][0] == RG.STRIP and e["cap"] is None)
    assert ro[j13] == 1 and st[j13] == 0


# ----------------------------------------------------------------------- 2. pairs
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_pairs(eng, route, profile):
    """Every ordered pair of {off, strip, wrap, dropped, source-skipped,
    caller-skipped} in one wave's two entries; n odd, the last entry alone."""
    room = ROOM[profile]
    fan = RedFan(RG.pairs(room), Peer([eng], RTP, profile, seed()), room)
    all_codes(fan)
    assert fan.n == 73
    seg, ln, st, ro = fan.held(eng, route)
    assert (st == N.STATUS_SKIPPED).sum() == 36 and ro[-1] == 1 and st[-1] == 0


@pytest.mark.parametrize("route", ["host", "device"])
def test_one_entry(eng, route):
    fan = RedFan([RG.entry(RG.packet(0x0ECF0001 + (route == "host"), 3, 50), (RG.STRIP, RG.RED_PT))],
                 Peer([eng], RTP, CM, seed()), 10)
    seg, ln, st, ro = fan.held(eng, route)
    assert (ro.tolist(), st.tolist(), ln.tolist()) == ([1], [0], [49 + 10])


# -------------------------------------------------------- 3. the reference's answers
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_reference_answers(eng, route, profile):
    """Multi-block: -1, SKIPPED and counted; PT mismatch, version 1, marker with
    PT 72..83: 0 and the _pay call's bytes; strip with h == c: -1; strip with
    h > c or a negative extension length: 0; wrap with h > c: -1; an extension
    length word past c: -1; a header's end at 0 and 4.  The stats move by
    red_ref's counts."""
    room = ROOM[profile]
    fan = RedFan(RG.answers(room), Peer([eng], RTP, profile, seed()), room)
    all_codes(fan)
    before = eng.fanout_red_stats()
    seg, ln, st, ro = fan.held(eng, route)
    after = eng.fanout_red_stats()
    assert ro.tolist() == [e["want"] for e in fan.grid]
    bad = [RG.malformed(e, room) for e in fan.grid]
    first = bad.index(True)  # from there on the chain ends the bundle, as the reference's loop does
    assert st[first] == N.STATUS_ERR_MALFORMED and set(st[first + 1:].tolist()) <= {N.STATUS_NOT_PROCESSED, N.STATUS_SKIPPED}
    assert N.STATUS_ERR_MALFORMED not in st[:first].tolist() and N.STATUS_NOT_PROCESSED not in st[:first].tolist()
    assert all(st[j] == N.STATUS_SKIPPED and ln[j] == 0 for j in np.nonzero(ro == -1)[0])
    assert after["calls"] == before["calls"] + 1
    for name, code in (("stripped", 1), ("wrapped", 2), ("dropped", -1)):
        assert after[name] - before[name] == int((fan.codes == code).sum()), name


# ------------------------------------------------------ 4. with the other records
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_with_the_other_records(eng, route, profile):
    """One entry per mode carrying all four records: a stamp whose walk reaches
    the four bytes past the extension (the kept quirk) and so reads the payload
    as RED left it, a patch at h and one across the piece boundary at 32, all
    four setters.  The expected fan's stamp landed where the moved bytes say."""
    room = ROOM[profile]
    fan = RedFan(RG.together(room), Peer([eng], RTP, profile, seed()), room)
    all_codes(fan)
    seg, ln, st, ro = fan.held(eng, route)
    assert ro.tolist() == [1, 2, -1, 0] and st.tolist() == [0, 0, N.STATUS_SKIPPED, 0]
    assert fan.g.at.tolist()[:2] == [21, 21] and fan.g.at[3] == 17
    # the same walk over the sources as they were finds nothing: the stamp depends on RED's move
    plain = PayFan([e["pkt"] for e in fan.grid[:2]], [(j, fan.f.peers[j]) for j in range(2)], None,
                   [e["ast"] for e in fan.grid[:2]], None)
    plain.expand()
    assert plain.at.tolist() == [-1, -1]


# ------------------------------------------------------------ 5. degenerate calls
@pytest.mark.parametrize("route", ["host", "device"])
def test_without_records_it_is_the_pay_call(engine_factory, oracle, route):
    """red = None against fanout_*_pay on an identical engine, and all-off
    records on a third: statuses, lengths and the destination bytes (device: the
    whole segment bit for bit; host: every OK region); red_out all 0."""
    engs = [make_engine(engine_factory) for _ in range(3)]
    peer = Peer(engs, RTP, CM, seed())
    grid = RG.together(10) + RG.pairs(10)[:24]
    off = [dict(e, red=(RG.OFF, 0)) for e in grid]
    a = RedFan(off, peer, 10, pass_red=False, which=0)
    want = a.f.run_host(engs[0]) if route == "host" else a.f.run_device(engs[0])
    a.f.check(engs[0], want, which=0)
    for k, fan in ((1, RedFan(off, peer, 10, pass_red=False, which=1)), (2, RedFan(off, peer, 10, which=2))):
        # the references have seen these packets once (above): this engine is held to the first one's output
        seg, ln, st, ro = fan.run_host(engs[k]) if route == "host" else fan.run_device(engs[k])
        assert ro.tolist() == ([77] * fan.n if k == 1 and route == "device" else [0] * fan.n)
        assert st.tolist() == want[2].tolist() and ln.tolist() == want[1].tolist()
        if route == "device":
            assert np.array_equal(seg, want[0])
        for j in np.nonzero(st == 0)[0]:
            o = int(fan.f.off[j])
            assert np.array_equal(seg[o:o + int(ln[j])], want[0][o:o + int(ln[j])]), j
        print("engine", k, engs[k].fanout_stats(), "engine 0", engs[0].fanout_stats(), "statuses", st.tolist())
        assert engs[k].fanout_stats() == engs[0].fanout_stats()
        assert engs[k].fanout_red_stats() == {"calls": k - 1, "stripped": 0, "wrapped": 0, "dropped": 0}


def test_record_alignment(eng):
    """A record array at a 4-byte (not 16-byte) offset runs; at a 1-byte offset
    the call is refused with nothing launched."""
    fan = RedFan(RG.answers(10), Peer([eng], RTP, CM, seed()), 10)
    all_codes(fan)
    fan.held(eng, "device", misalign=4)
    bad = RedFan(RG.answers(10), Peer([eng], RTP, CM, seed()), 10)
    st0, rs0 = eng.fanout_stats(), eng.fanout_red_stats()
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        bad.run_device(eng, misalign=1)
    assert (bad.seg_after == FILL).all() and (bad.ro_after == 77).all() and np.array_equal(bad.src_after, bad.f.src_seg)
    assert eng.fanout_stats() == st0 and eng.fanout_red_stats() == rs0


def test_host_refuses_out_of_range_records(eng):
    fan = RedFan(RG.answers(10)[:4], Peer([eng], RTP, CM, seed()), 10)
    st0 = eng.fanout_stats()
    for field, value in (("mode", 3), ("red_pt", 128), ("reserved", (1, 0)), ("reserved", (0, 1))):
        keep = fan.red.copy()
        fan.red[field][2] = value
        with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
            fan.run_host(eng)
        fan.red = keep
    assert eng.fanout_stats() == st0


def test_device_ignores_out_of_range_records(eng):
    """On the device route such a record switches its entry's step off."""
    grid = [RG.entry(RG.packet(0x0ECE0000 + j, 5, 60), (RG.STRIP, RG.RED_PT)) for j in range(5)]
    fan = RedFan([dict(e, red=(RG.OFF, 0)) if j < 4 else e for j, e in enumerate(grid)], Peer([eng], RTP, CM, seed()), 10)
    fan.red["mode"][:4], fan.red["red_pt"][:4] = [3, 1, 1, 255], [RG.RED_PT, 128, RG.RED_PT, RG.RED_PT]
    fan.red["reserved"][2] = (0, 1)
    seg, ln, st, ro = fan.held(eng, "device")
    assert ro.tolist() == [0, 0, 0, 0, 1] and ln.tolist() == [70, 70, 70, 70, 69]
