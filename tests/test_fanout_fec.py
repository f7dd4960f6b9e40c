"""Fan-out that makes ulpfec packets per destination (srtp_fanout_device_fec /
_host_fec, k_fanout_fec): a destination entry without a source becomes the
RFC 5109 packet over up to 16 member entries of the same call, as all their
records left them, and is protected like any other entry.

The expected result is the definition itself: fec_ref (FECSender.FECPacket's
addMedia and finish, and the RED wrap, restated from the Java) over the members
as red_ref, the setters, payload_ref and abs_send_time_ref leave them makes each
FEC packet on the host; it is submitted as an ordinary source in the FEC
entry's place, a refused entry is flagged SKIP, and that fan goes the way of
the other fan-out tests, through oracle.process / gcm_ref.process.  Every run
asserts bit equality of len, status, fec_out, the bytes [off, off + len) of
every OK entry and the context state and, on the device route, every FILL byte
outside the regions rounded up to 16 and in the regions of skipped and refused
entries, and the source segment.  One refusal leaves bytes behind and is held
to them instead: an FEC entry on the device route whose own src_idx names a
source was copied by the expansion before k_fanout_fec refused it.  The grids
are tests/fec_grids.py's, which a test without a GPU holds to the counts
asserted here."""
import numpy as np
import pytest

import fec_grids as FG
import fec_ref as F
import gcm_ref as G
import red_grids as RG
from libjitsi_amd import FecSender, RawPacket, fan_out_fec
from libjitsi_amd import _native as N
from oracle import oracle as O
from test_fanout import FILL, RTP, SKIP, Peer, make_engine, seed, up16
from test_fanout_ast import stamp
from test_fanout_pay import PayFan, pay
from test_fanout_rewrite import rec

pytestmark = pytest.mark.gpu

CM, GCM = "AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM"
ROOM = {CM: 10, GCM: 16}
INVALID, CAPACITY, SKIPPED = N.STATUS_DROP_INVALID, N.STATUS_ERR_CAPACITY, N.STATUS_SKIPPED
ROUTES = [(r, p) for r in ("host", "device") for p in (CM, GCM)]
IDS = ["%s-%s" % (r, "cm" if p == CM else "gcm") for r, p in ROUTES]


class FecFan:
    """A grid of fec_grids entries: `f` holds the arrays the engine gets, `g`
    the fan the references process, with every made FEC packet as a source of
    its own."""

    def __init__(self, grid, peers, room, gaps=(16, 48), pass_fec=True, which=0):
        self.grid, self.n, self.which, self.pass_fec, self.room = grid, len(grid), which, pass_fec, room
        codes, packets, self.member_bytes = FG.expect(grid, room)
        self.codes, self.packets = np.array(codes, np.int8), packets
        media = [j for j, e in enumerate(grid) if e["fec"] is None]
        src_of = {j: i for i, j in enumerate(media)}
        fec_src = {j: len(media) + x for x, j in enumerate(sorted(packets))}
        is_m = lambda j: grid[j]["fec"] is None
        caps = [FG.media_cap(e, room) if is_m(j) else FG.fec_cap(grid, j, room, packets) for j, e in enumerate(grid)]
        some = lambda k: any(e.get(k) is not None for e in grid)
        rws = [e.get("rw") or rec() for e in grid] if some("rw") else None
        asts = [e.get("ast") or stamp(0, 3, 0) for e in grid] if some("ast") else None
        pays = [e.get("pay") or pay() for e in grid] if some("pay") else None
        exp = {j: RG.expect(grid[j], room) for j in media}
        status = [grid[j]["status"] for j in media]
        ef, eg = [], []
        for j, e in enumerate(grid):
            p = peers[e["peer"]]
            if is_m(j):
                ef.append((src_of[j], p, caps[j], e["flags"]))
                eg.append((src_of[j], p, caps[j], e["flags"] | (SKIP if exp[j][0] < 0 else 0)))
            else:
                own = e["fec"]["src"]
                ef.append((-1 if own is None else src_of[own], p, caps[j], e["flags"]))
                eg.append((fec_src[j], p, caps[j], e["flags"]) if j in packets else (0, p, caps[j], e["flags"] | SKIP))
        self.f = PayFan([grid[j]["pkt"] for j in media], ef, rws, asts, pays, gaps=gaps, src_status=status)
        self.g = PayFan([exp[j][1] for j in media] + [packets[j] for j in sorted(packets)], eg, rws, asts, pays, gaps=gaps,
                        src_status=status + [0] * len(packets))
        assert np.array_equal(self.f.off, self.g.off) and self.f.seg_bytes == self.g.seg_bytes
        self.red = None
        if any(is_m(j) and e["red"][0] for j, e in enumerate(grid)):
            self.red = np.zeros(self.n, N.FANOUT_RED_DTYPE)
            for j in media:
                self.red[j] = (grid[j]["red"][0], grid[j]["red"][1], (0, 0))
        self.fec, self.members = FG.arrays(grid)
        self.copied_anyway = [j for j, e in enumerate(grid) if not is_m(j) and e["fec"]["src"] is not None]

    def run_host(self, eng):
        f = self.f
        seg = np.full(f.seg_bytes, FILL, np.uint8)
        src = f.src_seg.copy()
        ln, st, ro, fo = eng.fanout_host_fec(f.tids, f.src_seg, f.src_off, f.src_len, f.src_cap, f.src_idx, seg, f.off,
                                             f.cap, f.src_status, f.flags if f.flags.any() else None, f.records(),
                                             f.stamps(), f.pays(), self.red, self.fec if self.pass_fec else None,
                                             self.members if self.pass_fec else None)
        assert np.array_equal(src, f.src_seg)
        return seg, ln, st, fo

    def run_device(self, eng, misalign=0, fec_out=True):
        import torch
        f = self.f
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

        def records(arr, size, shift=0):
            if arr is None:
                return None
            blob = arr.view(np.uint8).reshape(-1).copy()
            raw = torch.zeros(len(blob) + 32, dtype=torch.uint8, device="cuda")
            raw[shift:shift + len(blob)].copy_(torch.from_numpy(blob))
            return raw[shift:shift + len(blob)]
        src_seg = d(f.src_seg)
        seg = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
        fo = torch.full((f.n,), 77, dtype=torch.int8, device="cuda")
        args = [d(f.src_off), d(f.src_len), d(f.src_cap), d(f.src_idx), seg, d(f.off), ln, d(f.cap), st]
        rw, ast, py, red = records(f.records(), 16), records(f.stamps(), 8), records(f.pays(), 8), records(self.red, 4)
        fec = records(self.fec if self.pass_fec else None, 12, misalign)
        mem = records(self.members if self.pass_fec and len(self.members) else None, 4, misalign)
        src_status = None if f.src_status is None else d(f.src_status)
        flags = d(f.flags) if f.flags.any() else None
        torch.cuda.synchronize()
        try:
            eng.fanout_device_fec(d(f.tids), src_seg, *args, rw, ast, py, red, None, fec, mem, fo if fec_out else None,
                                  src_status=src_status, flags=flags, n_members=len(self.members) if self.pass_fec else 0)
        finally:
            eng.sync(None)
            torch.cuda.synchronize()
            self.src_after = src_seg.cpu().numpy()
            self.seg_after = seg.cpu().numpy()
            self.fo_after = fo.cpu().numpy()
        return self.seg_after, ln.cpu().numpy().view(np.uint32), st.cpu().numpy(), self.fo_after

    def held(self, eng, route, **kw):
        f, g = self.f, self.g
        seg, ln, st, fo = self.run_host(eng) if route == "host" else self.run_device(eng, **kw)
        for j in np.nonzero(self.fec["mode"])[0]:
            print("entry %3d: fec count %2d mode %d code %2d/%2d len %5d cap %5d status %d" % (
                j, self.fec["count"][j], self.fec["mode"][j], fo[j], self.codes[j], ln[j], f.cap[j], st[j]))
        assert fo.tolist() == (self.codes.tolist() if self.pass_fec else [0 if route == "host" else 77] * self.n)
        g.check(eng, (seg, ln, st), which=self.which)
        if route == "device":
            want = g.expand()[0]
            inside = np.zeros(f.seg_bytes, bool)
            for j in range(self.n):
                o, c = int(f.off[j]), up16(f.cap[j])
                if j in self.copied_anyway:  # refused behind the expansion's copy: skipped, the copy left there
                    k = up16(min(int(f.src_len[f.src_idx[j]]), int(f.cap[j])))
                    assert st[j] == SKIPPED and ln[j] == 0 and (seg[o + k:o + c] == FILL).all(), j
                    inside[o:o + c] = True
                    continue
                if g.skipped(j)[0]:  # skipped, dropped by RED or refused: nothing is written
                    assert st[j] == SKIPPED and ln[j] == 0 and (seg[o:o + c] == FILL).all(), j
                    continue
                inside[o:o + c] = True
                if self.grid[j]["fec"] is None and self.grid[j]["red"][0] == RG.WRAP and ln[j] > f.cap[j]:
                    assert st[j] == INVALID and (seg[o:o + c] == FILL).all(), j  # a wrap that does not fit
                elif st[j] in (INVALID, N.STATUS_NOT_PROCESSED):  # the chain left the entry as it was made
                    k = max(g.copied(j), 0)
                    assert np.array_equal(seg[o:o + k], want[o:o + k]), j
                    assert (seg[o + up16(k):o + c] == FILL).all(), j
            assert (seg[~inside] == FILL).all()
            assert np.array_equal(self.src_after, f.src_seg)
        return seg, ln, st, fo


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


def counted(eng, fan, route, **kw):
    """held(), with the stats deltas: fec_ref's counts, and `skipped` as if the FEC entries had sources."""
    before, sk = eng.fanout_fec_stats(), eng.fanout_stats()["skipped"]
    got = fan.held(eng, route, **kw)
    after = eng.fanout_fec_stats()
    delta = {k: after[k] - before[k] for k in after}
    print("stats delta", delta, "member bytes by fec_ref", fan.member_bytes)
    assert delta == {"calls": 1, "made": int((fan.codes == 1).sum()), "refused": int((fan.codes == -1).sum()),
                     "member_bytes": fan.member_bytes}
    # what still counts: a source that was not OK, and an entry without a source whose record is off
    by_source = sum(1 for e in fan.grid if (e["status"] != 0 if e["fec"] is None else e["fec"]["mode"] == 0))
    assert eng.fanout_stats()["skipped"] - sk == by_source
    return got


# ------------------------------------------------------------------ 1. boundaries
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_boundaries(eng, route, profile):
    """fec_grids.boundaries: every length list as a group, plain and wrapped, into destinations that fit exactly,
    lack the trailer's room (ERR_CAPACITY) and are a byte short (DROP_INVALID); every length as a group's longest
    (the packet's end around bytes 32, 48, 64, 1024 and 2048); counts 1, 2, 3, 15, 16 over sequence numbers that
    wrap; mixed lengths; members with CSRCs and an extension."""
    room = ROOM[profile]
    fan = FecFan(FG.boundaries(room), [Peer([eng], RTP, profile, seed())], room)
    seg, ln, st, fo = counted(eng, fan, route)
    tight = [j for j, e in enumerate(fan.grid) if e["fec"] is not None and e["cap"] is not None]
    assert len(tight) == 24
    for j in tight:
        size = len(fan.packets[j])
        want = {size + room: 0, size: CAPACITY, size - 1: INVALID}[fan.grid[j]["cap"]]
        assert (fo[j], st[j], ln[j]) == (1, want, size + (room if want == 0 else 0)), j
    assert (fo == 1).sum() == 96 and ((fo == 1) & (st == 0)).sum() == 96 - 16 and (fo == -1).sum() == 1
    ends = {int(ln[j]) - room for j in np.nonzero((fo == 1) & (st == 0))[0]}
    assert {1022, 1023, 1024, 1025, 1026, 1027, 2046, 2047, 2048, 2049, 2050, 2051} <= ends and {26, 27, 31, 32} <= ends


# ---------------------------------------------------------- 2. members with records
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_members_with_records(eng, route, profile):
    """All four setters, a stamp, both patches and RED strip and wrap on the members: the XOR is over the final
    bytes.  The same sources toward two peers with different rewrites give different FEC packets."""
    room = ROOM[profile]
    peers = [Peer([eng], RTP, profile, seed()) for _ in range(2)]
    fan = FecFan(FG.with_records(room), peers, room)
    assert fan.red is not None and fan.f.records() is not None and fan.f.pays() is not None and fan.f.stamps() is not None
    seg, ln, st, fo = counted(eng, fan, route)
    made = [j for j in np.nonzero(fo == 1)[0]]
    assert len(made) == 4 and all(st[j] == 0 for j in made)
    a, b = (fan.packets[j] for j in made if fan.grid[j]["fec"]["mode"] == FG.PLAIN)
    assert a != b and a[26:] != b[26:] and len(a) == len(b)
    # the members' plaintext the references were given is fec_grids' own restatement of it
    want = fan.g.expand()[0]
    for j, e in enumerate(fan.grid):
        if e["fec"] is None and FG.final(e, room)[0] is not None:
            o = int(fan.f.off[j])
            assert bytes(want[o:o + FG.final(e, room)[1]]) == FG.final(e, room)[0], j


# -------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_refusals(eng, route, profile):
    """One entry per refusal cause among entries that are made.  The device route takes the out-of-range fields
    and indices too and refuses those entries; the host route's grid holds the causes a running call can meet."""
    room = ROOM[profile]
    grid = FG.refusals(room, route == "device")
    fan = FecFan(grid, [Peer([eng], RTP, profile, seed())], room)
    seg, ln, st, fo = counted(eng, fan, route)
    assert all(st[j] == SKIPPED and ln[j] == 0 for j in np.nonzero(fo == -1)[0])
    assert all(st[j] == 0 for j in np.nonzero(fo == 1)[0])
    assert ((fo == 1).sum(), (fo == -1).sum()) == ((5, 16) if route == "device" else (3, 6))
    if route == "device":
        assert len(fan.copied_anyway) == 1


def test_host_refuses_what_the_rule_would(eng):
    """Host route: every record or member the rule refuses for its fields or indices is SRTP_EINVAL with nothing
    launched; neither stats move."""
    room = ROOM[CM]
    peer = Peer([eng], RTP, CM, seed())
    s0, f0 = eng.fanout_stats(), eng.fanout_fec_stats()
    good = lambda: FG.stream((50, 60, 70, 80)) + [FG.fec([0, 1]), FG.fec([0, 1, 2])]
    FecFan(good(), [peer], room).held(eng, "host")
    s1, f1 = eng.fanout_stats(), eng.fanout_fec_stats()
    assert s1["calls"] == s0["calls"] + 1 and f1["made"] == f0["made"] + 2
    bad = FG.field_refusals(5) + [FG.fec([0, 1], mode=0)]  # an off record without a source: -1 is for records that are on
    assert len(bad) == 11
    for b in bad:
        grid = good() + [b]
        assert b["fec"]["mode"] == 0 or FG.field_causes(grid, 6)
        with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
            FecFan(grid, [peer], room).run_host(eng)
    s0, f0 = s1, f1
    assert eng.fanout_stats() == s0 and eng.fanout_fec_stats() == f0


# ------------------------------------------------ 4. shared members and many entries
@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_shared_members(eng, route, profile):
    """Nine packets in three rows and three columns: six FEC entries, every packet in two of them."""
    room = ROOM[profile]
    fan = FecFan(FG.shared(room), [Peer([eng], RTP, profile, seed())], room)
    seg, ln, st, fo = counted(eng, fan, route)
    assert (fo == 1).sum() == 6 and all(st[j] == 0 for j in np.nonzero(fo == 1)[0])


@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
@pytest.mark.parametrize("n_fec", [1, 130])
def test_many_entries(eng, route, profile, n_fec):
    room = ROOM[profile]
    fan = FecFan(FG.many(n_fec), [Peer([eng], RTP, profile, seed())], room)
    seg, ln, st, fo = counted(eng, fan, route)
    assert (fo == 1).sum() == n_fec and (st[fo == 1] == 0).all() and fan.n == 3 * n_fec + 3


@pytest.mark.parametrize("route", ["host", "device"])
def test_all_refused(eng, route):
    fan = FecFan(FG.all_refused(10), [Peer([eng], RTP, CM, seed())], 10)
    seg, ln, st, fo = counted(eng, fan, route)
    assert fo.tolist() == [0] * 3 + [-1] * 5 and set(st.tolist()) == {SKIPPED} and not ln.any()


@pytest.mark.parametrize("route", ["host", "device"])
def test_second_trip_of_the_stride_loop(eng, route):
    """More entries than the launch has waves (4096 blocks of four): the waves that take a second entry find an
    FEC entry there, behind 16384 entries of which the first are FEC entries too."""
    head = FG.many(4)[:12]
    ssrc = 0x0FECAAAA
    body = FG.stream([12] * (16384 - len(head) + 6), seq=0, ssrc=ssrc)
    at = len(head) + len(body)
    grid = head + body + [FG.fec([at - 2, at - 1]), FG.fec([at - 4, at - 3, 0], FG.RED)]
    assert len(grid) == 16384 + 8 and grid[16384 + 6]["fec"] is not None
    fan = FecFan(grid, [Peer([eng], RTP, CM, seed())], 10, gaps=(0,))
    seg, ln, st, fo = counted(eng, fan, route)
    assert (fo == 1).sum() == 6 and fo[-2:].tolist() == [1, 1] and st[-2:].tolist() == [0, 0]


# ------------------------------------------------------------ 5. order and recovery
def stream_grid(shift, start=0xFFFA, mode=FG.PLAIN):
    """Eight packets of one SSRC at rate 4, each group followed by its FEC entry under the same SSRC; with the
    shift, the second group's sequence numbers are rewritten one up, past the first FEC packet's."""
    ssrc = FG._next()
    g = []
    for grp in range(2):
        at = len(g)
        for i in range(4):
            seq = (start + 4 * grp + i) & 0xFFFF
            e = FG.media(RG.packet(ssrc, seq, 60 + 9 * i + grp, pt=100))
            if shift and grp:
                e["rw"] = (N.REWRITE_SEQ, 0, 0, (seq + grp) & 0xFFFF, 0, 0)
            g.append(e)
        g.append(FG.fec(range(at, at + 4), mode, ssrc=ssrc))
    return g, ssrc


@pytest.mark.parametrize("route,profile", ROUTES, ids=IDS)
def test_order_and_recovery(eng, route, profile):
    """Shifted sequence numbers across the 16-bit wrap: every status OK, ROC 1.  The receiving side unprotects
    all packets with the references, loses one media packet per group, and RFC 5109's recovery gives its
    plaintext back."""
    room = ROOM[profile]
    s = seed()
    peer = Peer([eng], RTP, profile, s)
    grid, ssrc = stream_grid(True)
    fan = FecFan(grid, [peer], room)
    seg, ln, st, fo = fan.held(eng, route)
    assert st.tolist() == [0] * 10 and fo.tolist() == [0, 0, 0, 0, 1] * 2
    seqs = [int.from_bytes(fan.g.expand()[0][int(o) + 2:int(o) + 4].tobytes(), "big") for o in fan.f.off]
    assert seqs == [0xFFFA, 0xFFFB, 0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF, 0, 1, 2, 3]
    state = eng.context_state(peer.e[0], ssrc)
    assert int(state["roc"]) == 1 and int(state["s_l"]) == 3
    rcv = Peer([eng], RTP, profile, s, sender=False)  # the same keys, the receiving side
    back, ln_b = seg.copy(), ln.copy()
    proc = G.process if rcv.gcm else O.process
    st_b = proc([rcv.r] * 10, True, back, fan.f.off, ln_b, fan.f.cap, np.zeros(10, np.uint32), True)
    assert st_b.tolist() == [0] * 10
    plain = [bytes(back[int(o):int(o) + int(L)]) for o, L in zip(fan.f.off, ln_b)]
    for grp, lost in ((0, 2), (1, 0)):
        media, fec = plain[5 * grp:5 * grp + 4], plain[5 * grp + 4]
        assert fec == fan.packets[5 * grp + 4]
        got = F.recover(fec, [p for i, p in enumerate(media) if i != lost])
        assert got == media[lost], (grp, lost)


@pytest.mark.parametrize("route", ["host", "device"])
def test_without_the_shift_a_number_is_used_twice(eng, route):
    """Without the shift the second group's first packet carries the first FEC packet's sequence number under the
    same SSRC: the references, and so the engine, answer it as they answer any number used twice."""
    grid, ssrc = stream_grid(False, start=500)
    fan = FecFan(grid, [Peer([eng], RTP, CM, seed())], 10)
    seg, ln, st, fo = fan.held(eng, route)
    print("statuses", st.tolist())
    assert fo.tolist() == [0, 0, 0, 0, 1] * 2
    assert st.tolist() == [0] * 5 + [N.STATUS_DROP_REPLAY] + [0] * 4


# ------------------------------------------------------------ 6. degenerate calls
@pytest.mark.parametrize("route", ["host", "device"])
def test_without_records_it_is_the_red_call(engine_factory, oracle, route):
    """fec = None against fanout_*_red on an identical engine, and all-off records on a third: statuses, lengths
    and the destination bytes (device: the whole segment bit for bit); fec_out all 0."""
    import test_fanout_red as TR
    engs = [make_engine(engine_factory) for _ in range(3)]
    peer = Peer(engs, RTP, CM, seed())
    rgrid = RG.together(10) + RG.pairs(10)[:24]
    a = TR.RedFan(rgrid, peer, 10, which=0)
    want = a.run_host(engs[0]) if route == "host" else a.run_device(engs[0])
    a.g.check(engs[0], want[:3], which=0)
    grid = [dict(e, fec=None, peer=0) for e in rgrid]
    for k, pass_fec in ((1, False), (2, True)):
        fan = FecFan(grid, [peer], 10, pass_fec=pass_fec, which=k)
        assert np.array_equal(fan.f.off, a.f.off) and not fan.fec["mode"].any()
        seg, ln, st, fo = fan.run_host(engs[k]) if route == "host" else fan.run_device(engs[k])
        assert fo.tolist() == ([77] * fan.n if k == 1 and route == "device" else [0] * fan.n)
        assert st.tolist() == want[2].tolist() and ln.tolist() == want[1].tolist()
        if route == "device":
            assert np.array_equal(seg, want[0])
        for j in np.nonzero(st == 0)[0]:
            o = int(fan.f.off[j])
            assert np.array_equal(seg[o:o + int(ln[j])], want[0][o:o + int(ln[j])]), j
        assert engs[k].fanout_stats() == engs[0].fanout_stats()
        assert engs[k].fanout_red_stats() == engs[0].fanout_red_stats()
        assert engs[k].fanout_fec_stats() == {"calls": k - 1, "made": 0, "refused": 0, "member_bytes": 0}


def test_record_alignment(eng):
    """Record and member arrays at a 4-byte (not 16-byte) offset run; at a 1-byte offset the call is refused with
    nothing launched.  fec_out may be left out."""
    fan = FecFan(FG.shared(10), [Peer([eng], RTP, CM, seed())], 10)
    fan.held(eng, "device", misalign=4)
    bad = FecFan(FG.shared(10), [Peer([eng], RTP, CM, seed())], 10)
    st0, fs0 = eng.fanout_stats(), eng.fanout_fec_stats()
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        bad.run_device(eng, misalign=1)
    assert (bad.seg_after == FILL).all() and (bad.fo_after == 77).all() and np.array_equal(bad.src_after, bad.f.src_seg)
    assert eng.fanout_stats() == st0 and eng.fanout_fec_stats() == fs0
    quiet = FecFan(FG.shared(10), [Peer([eng], RTP, CM, seed())], 10)
    seg, ln, st, fo = quiet.run_device(eng, fec_out=False)
    assert (fo == 77).all()
    quiet.g.check(eng, (seg, ln, st))


# ------------------------------------------------------------------ 7. fan_out_fec
def test_fan_out_fec_api(engine_factory, oracle):
    """fan_out_fec end to end: three peers, one with a plain sender at rate 3 and a rewriter, one with a wrapped
    sender at rate 2, one without; against each peer's own transform() on a twin engine of packets made on the
    host with fec_ref.  A second call goes on from nb_fec."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    peers = [Peer([e1, e2], RTP, name, seed()) for name in (CM, GCM, CM)]
    A = 0x0FEC5000
    raw = [RG.packet(A, 0xFFFB + i, 70 + 11 * i, pt=100) for i in range(4)] + [RG.packet(A, i - 1, 90 + i, pt=100) for i in range(1, 4)]
    senders = [FecSender(A + 1, 3, 116), FecSender(A, 2, 117, 96), None]
    rewriter = lambda p: {"ssrc": A + 1, "timestamp": p.readInt(4) + 5}

    def expected(k, pkts, nb0):
        """What peer k is sent: (media per packet, [(i, fec packet)]) by the setters and fec_ref."""
        snd, out, fecs, group, nb = senders[k], [], [], [], nb0
        for i, r in enumerate(pkts):
            b = bytearray(r)
            if k == 0:
                FG.setters(b, (N.REWRITE_SSRC | N.REWRITE_TIMESTAMP, A + 1, int.from_bytes(r[4:8], "big") + 5, 0, 0))
            if snd is not None:
                FG.setters(b, (N.REWRITE_SEQ, 0, 0, int.from_bytes(r[2:4], "big") + nb, 0))
                group.append(bytes(b))
            out.append(bytes(b))
            if snd is not None and (len(group) == snd.rate or (group and i == len(pkts) - 1)):
                fecs.append((i, F.make(group, snd.ssrc, snd.pt, snd.red_pt)))
                group, nb = [], nb + 1
        return out, fecs

    nb = [0, 0, 0]
    for call, part in enumerate((raw[:5], raw[5:])):
        pkts = [RawPacket(r, 0, len(r)) for r in part]
        out, codes, fec = fan_out_fec(pkts, [p.e[0] for p in peers], [rewriter, None, None], [None] * 3, [None] * 3,
                                      [None] * 3, senders)
        assert codes == [[0] * len(part)] * 3
        for k, p in enumerate(peers):
            media, fecs = expected(k, part, nb[k])
            assert [i for i, _ in fec[k]] == [i for i, _ in fecs], (call, k)
            order = []  # the peer's packets in the order of the call's entries: media first, then its FEC packets
            order += [(out[k][i], media[i]) for i in range(len(part))]
            order += [(got, want) for (_, got), (_, want) in zip(fec[k], fecs)]
            want = p.e[1].transform([RawPacket(w, 0, len(w)) for _, w in order])
            for (got, plain), w in zip(order, want):
                assert got is not None and got.data() == w.data(), (call, k, len(plain))
            nb[k] += len(fecs)
    assert (senders[0].counter, senders[0].nb_fec, senders[1].counter, senders[1].nb_fec) == (7, 3, 7, 4)
