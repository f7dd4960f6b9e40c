"""Fan-out that stamps abs-send-time (srtp_fanout_device_ast / _host_ast,
k_fanout_ast, fan_out_ast()): each destination entry carries an 8-byte record
(value, id, on); where the copy holds a one-byte header-extension element with
that ID, found as AbsSendTimeEngine.replaceAbsSendTime finds it, its three data
bytes become the value before the protect chain runs.

The expected result is built as for fan-out with rewriting: the entries are
expanded on the host with numpy, each host-made copy of c >= 12 bytes is
stamped by abs_send_time_ref (the Java method restated over a bytearray of
exactly the c bytes), rewritten by RawPacket's four setters where a rewrite
record is present, and that bundle goes through the references
(oracle.process, gcm_ref.process).  Compared: status and length of every entry,
every byte of every OK region, the pre-protect bytes of the entries that end
DROP_INVALID (device route), guard bytes around every region, the source
segment before and after, and the contexts' state.

A stamp in piece 0 (bytes 0..15) is not reachable: with no CSRC the first
element's data starts at byte 17.  So the setters' piece and the stamp's never
coincide; CC = 0 with the element first (bytes 17..19, piece 1) is the nearest
case and is covered with all four fields rewritten."""
import numpy as np
import pytest

import abs_send_time_ref as A
import gcm_ref as G
from libjitsi_amd import RawPacket, SRTPPolicy, abs_send_time, fan_out_ast, fan_out_rw
from libjitsi_amd import _native as N
from oracle import oracle as O
from test_fanout import FILL, KEYS_RTP, RTCP, RTP, SKIP, Peer, make_engine, seed, up16
from test_fanout_ast_host import RECORDS, packets
from test_fanout_rewrite import RwFan, distinct, rec, setters
import test_fanout as TF

pytestmark = pytest.mark.gpu

CM = "AES_CM_128_HMAC_SHA1_80"
INVALID = N.STATUS_DROP_INVALID
EL = b"\x32\xA0\xA1\xA2"  # ID 3, len field 2


def stamp(value=0, ext_id=3, on=1, reserved=0):
    return (value, ext_id, on, reserved)


def value_of(j):
    """A 24-bit value whose bytes are distinct, none zero, and change with j."""
    return ((0xC1 + j) & 0xFF | 1) << 16 | ((0x52 + 3 * j) & 0xFF | 2) << 8 | ((0xE3 + 7 * j) & 0xFF | 4)


def reseq(p, ssrc, seq):
    """The packet under another SSRC and sequence number (only packets of 12 bytes and more)."""
    return p[:2] + (seq & 0xFFFF).to_bytes(2, "big") + p[4:8] + ssrc.to_bytes(4, "big") + p[12:] if len(p) >= 12 else p


class AstFan(RwFan):
    """RwFan with one stamp record per entry.  records None: no rewrite array is passed."""

    def __init__(self, pkts, entries, records, stamps, **kw):
        super().__init__(pkts, entries, records if records is not None else [rec()] * len(entries), **kw)
        self.pass_records = records is not None
        assert len(stamps) == self.n
        self.ast = np.array([tuple(s) for s in stamps], N.FANOUT_AST_DTYPE).reshape(self.n)
        self.pass_stamps = True
        self.at = np.full(self.n, -1)  # where the reference stamped each copy

    def expand(self, rounded=False):
        seg, ln, fl = super().expand(rounded)
        for j in range(self.n):
            c = self.copied(j)
            if c >= 12:
                o = int(self.off[j])
                buf = bytearray(seg[o:o + c].tobytes())
                self.at[j] = A.apply(buf, self.ast[j])
                seg[o:o + c] = np.frombuffer(bytes(buf), np.uint8)
        return seg, ln, fl

    def stamps(self):
        return self.ast if self.pass_stamps else None

    def run_host(self, eng):
        seg = np.full(self.seg_bytes, FILL, np.uint8)
        src = self.src_seg.copy()
        ln, st = eng.fanout_host_ast(self.tids, self.src_seg, self.src_off, self.src_len, self.src_cap, self.src_idx,
                                     seg, self.off, self.cap, self.src_status,
                                     self.flags if self.flags.any() else None, self.records(), self.stamps())
        assert np.array_equal(src, self.src_seg)
        return seg, ln, st

    def run_device(self, eng, stream=None, misalign=0):
        import torch
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        src_seg = d(self.src_seg)
        seg = torch.full((self.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        args = [d(self.src_off), d(self.src_len), d(self.src_cap), d(self.src_idx), seg, d(self.off), ln, d(self.cap), st]
        rw = None if self.records() is None else torch.from_numpy(self.rw.view(np.uint8).copy()).cuda()
        ast = None
        if self.stamps() is not None:
            raw = torch.zeros(8 * self.n + 16, dtype=torch.uint8, device="cuda")
            ast = raw[misalign:misalign + 8 * self.n]
            ast.copy_(torch.from_numpy(self.ast.view(np.uint8).copy()))
        src_status = None if self.src_status is None else d(self.src_status)
        flags = d(self.flags) if self.flags.any() else None
        torch.cuda.synchronize()
        try:
            eng.fanout_device_ast(d(self.tids), src_seg, *args, rw, ast, src_status=src_status, flags=flags,
                                  stream=stream)
        finally:
            eng.sync(stream)
            torch.cuda.synchronize()
            self.src_after = src_seg.cpu().numpy()
            self.seg_after = seg.cpu().numpy()
        return self.seg_after, ln.cpu().numpy().view(np.uint32), st.cpu().numpy()

    def run(self, eng, route):
        return self.run_host(eng) if route == "host" else self.run_device(eng)

    def held(self, eng, route, ref=None):
        """Run on `route` and hold the result to the references; on the device
        route also the guard bytes, the regions of skipped entries, the copies
        the chain refused or, behind a throw, never reached (as they were
        expanded) and the source segment."""
        got = self.run(eng, route)
        ref = self.check(eng, got, ref)
        if route == "device":
            seg, _, st = got
            want = self.expand(rounded=True)[0]
            inside = np.zeros(self.seg_bytes, bool)
            for j in range(self.n):
                o, c = int(self.off[j]), up16(self.cap[j])
                if self.skipped(j)[0]:
                    assert st[j] == N.STATUS_SKIPPED and (seg[o:o + c] == FILL).all(), j
                    continue
                inside[o:o + c] = True
                if st[j] in (INVALID, N.STATUS_NOT_PROCESSED):  # the chain left the copy as it was expanded
                    k = up16(max(self.copied(j), 0))
                    assert np.array_equal(seg[o:o + k], want[o:o + k]), (j, self.ast[j])
                    assert (seg[o + k:o + c] == FILL).all(), j
            assert (seg[~inside] == FILL).all()
            assert np.array_equal(self.src_after, self.src_seg)
        return got, ref


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


_ssrc = [0x0A570000]


def fresh_ssrc():
    _ssrc[0] += 1
    return _ssrc[0]


def all_packets():
    return list(packets())


# --------------------------------------------------- 1. placement, CSRCs, positions
GROUPS = {"cc0": (0, 81), "cc1": (81, 162), "cc15": (162, 243)}


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_placement_and_positions(eng, route, group):
    """Behind 0, 1 and 15 CSRCs: the first stamped byte on every residue mod 16
    of the piece pairs 0/1, 1/2, 63/64 (lane 63's first load against lane 0's
    second) and 127/128 (first against second trip), residues 14 and 15
    straddling two pieces; then the element behind one element of every len
    0..15, and alone.  One peer, one entry per packet, a value of its own."""
    lo, hi = GROUPS[group]
    pk = all_packets()[lo:hi]
    assert len(pk) == 81
    peer = Peer([eng], RTP, CM, seed())
    ssrc = fresh_ssrc()
    src = [reseq(p, ssrc, 10 + i) for i, (p, _) in enumerate(pk)]
    f = AstFan(src, [(i, peer) for i in range(len(src))], None, [stamp(value_of(i)) for i in range(len(src))],
               gaps=(16, 48), room=10)
    (seg, ln, st), _ = f.held(eng, route)
    assert st.tolist() == [0] * f.n
    assert f.at.tolist() == [a for _, a in pk]  # the reference stamped where the packet was built to be stamped
    res = {(int(a) % 16, int(a) // 16) for a in f.at[:64]}
    assert {r for r, _ in res} == set(range(16))
    far = {q for r, q in res if r >= 14}  # the pieces a straddling stamp starts in
    assert far >= {63, 127} and len(far) >= 3 and (group != "cc0" or 1 in far)
    for j in range(f.n):  # the bytes themselves, not only through the reference
        o = int(f.off[j]) + int(f.at[j])
        assert seg[o:o + 3].tobytes() == value_of(j).to_bytes(3, "big"), j


# -------------------------------------------------------------------- 2. the quirks
@pytest.mark.parametrize("route", ["host", "device"])
def test_reference_quirks(eng, route):
    """Every quirk packet of the sweep (length bytes >= 0x80, length 0 and 1, a
    length beyond the packet, other profile words, V != 2, X clear, 15 CSRCs
    claimed, a match in the four overshoot bytes and behind them, one to six
    padding bytes in front, a first match with len != 2, a header that claims
    more than the packet holds) toward eight peers, one per record of the
    sweep: on, on with the ignored fields set, off, ID 16, ID 255, ID 0
    (against padding), an ID whose first element has another len, on = 2."""
    pk = all_packets()[243:]
    peers = [Peer([eng], RTP, CM, seed()) for _ in RECORDS]
    ssrc = fresh_ssrc()
    src = [reseq(p, ssrc, 10 + i) for i, (p, _) in enumerate(pk)]
    entries = [(i, p) for i in range(len(src)) for p in peers]
    stamps = [(value_of(i) | (r[0] & 0xFF000000),) + tuple(r[1:]) for i in range(len(src)) for r in RECORDS]
    f = AstFan(src, entries, None, stamps, gaps=(16, 48), room=10)
    (seg, ln, st), ref = f.held(eng, route)
    at = f.at.reshape(len(src), len(RECORDS))
    assert (at[:, 2:5] == -1).all()                       # off, ID 16, ID 255
    assert (at[:, 0] == at[:, 1]).all() and (at[:, 0] >= 0).sum() >= 10 and (at[:, 0] < 0).sum() >= 30  # quirks both ways
    assert (at[:, 5] == -1).all() and (at[:, 6] == -1).all()  # ID 0 and ID 5 never meet a len of 2 here
    exp = f.expand()[0]
    for j in np.nonzero(f.at < 0)[0]:  # an unstamped copy is the source, byte for byte
        c, si = f.copied(j), int(f.src_idx[j])
        if c > 0:
            assert exp[int(f.off[j]):][:c].tobytes() == src[si][:c]


# --------------------------------------------------------------------- 3. the cuts
@pytest.mark.parametrize("route", ["host", "device"])
def test_cut_by_the_end(eng, route):
    """The element at bytes 22..25 (stamp at 23): sources whose length ends the
    packet at p + 3 == B (not stamped) and p + 3 == B - 1 (stamped), and around;
    destinations whose capacity does (those end DROP_INVALID: the copy is held
    to the expanded bytes); a destination below the element's offset; c < 12
    through the source's length and through the destination's capacity."""
    body = A.one_byte_ext([(5, b"abcde"), (3, b"\xA0\xA1\xA2"), (7, b"pq")])
    at = 16 + 6 + 1
    peer = Peer([eng], RTP, CM, seed())
    ssrc = fresh_ssrc()
    cuts = [at - 3, at - 1, at, at + 1, at + 2, at + 3, at + 4, 11, 12]
    own = [Peer([eng], RTP, CM, seed()) for _ in cuts]  # a cut packet may throw: a transformer of its own
    base = [reseq(A.rtp_ext(1, 1, body, bytes(range(30))), ssrc, 10 + i) for i in range(2 * len(cuts) + 1)]
    src_len = [len(base[0])] * len(base)
    entries = []
    for i, c in enumerate(cuts):
        src_len[i] = c
        entries.append((i, own[i]))                     # the packet ends there
        entries.append((len(cuts) + i, peer, c))        # the destination does
    entries.append((len(base) - 1, peer))
    f = AstFan(base, entries, None, [stamp(value_of(j)) for j in range(len(entries))], gaps=(16, 48),
               src_len=src_len, room=10)
    (seg, ln, st), _ = f.held(eng, route)
    want = [a if c > at + 2 else -1 for c in cuts for a in (at, at)] + [at]
    assert f.at.tolist() == want
    assert [int(s) for s in st[1::2]] == [INVALID] * len(cuts) and st[-1] == 0


# -------------------------------------------------------------------- 4. the pairs
@pytest.mark.parametrize("n", [21, 1])
def test_pairs(engine_factory, oracle, n):
    """Wave pairs (entries 2k, 2k + 1): different IDs and values in one pair; one
    of the two off; one skipped by its flag, by its index and by its source's
    status; one whose region holds no byte, and 8 bytes -- each in both orders;
    an odd number of entries, and a single one.  The partners' records are on
    and must reach nothing but their own copy.  Device route (the host route
    refuses an index that names no source); then the host route without that
    pair."""
    e1 = make_engine(engine_factory)
    a, b = (Peer([e1], RTP, CM, seed()) for _ in range(2))
    ssrc = fresh_ssrc()
    two = A.one_byte_ext([(4, b"\xB0\xB1\xB2"), (3, b"\xA0\xA1\xA2")])  # ID 4 at 17, ID 3 at 21
    pk = [reseq(A.rtp_ext(1, 1, two, G.payload(L, i)), ssrc, 10 + i) for i, L in enumerate((4, 100, 17, 1200, 64, 40))]
    status = [0, 0, 0, 0, 0, N.STATUS_DROP_AUTH]
    K = SKIP
    # (source, peer, cap, flags, (id, on))
    pairs = [((0, a, None, 0, (3, 1)), (0, b, None, 0, (4, 1))), ((1, a, None, 0, (4, 1)), (1, b, None, 0, (3, 0))),
             ((2, a, None, 0, (3, 0)), (2, b, None, 0, (4, 1))), ((3, a, None, 0, (3, 1)), (3, b, None, K, (3, 1))),
             ((4, a, None, K, (4, 1)), (4, b, None, 0, (4, 1))), ((5, a, None, 0, (3, 1)), (0, a, None, 0, (4, 1))),
             ((1, a, None, 0, (3, 1)), (5, b, None, 0, (3, 1))), ((2, a, None, 0, (4, 1)), (1000, b, 64, 0, (3, 1))),
             ((-1, a, 64, 0, (3, 1)), (3, a, None, 0, (4, 1))), ((4, a, None, 0, (3, 1)), (1, b, 0, 0, (3, 1))),
             ((2, b, 8, 0, (3, 1)), (3, b, None, 0, (3, 1)))]
    flat = [e for pr in pairs for e in pr][:n] if n > 1 else [pairs[0][1]]
    # sources 0, 1, 2, 3, 4 go to peer a twice: give the repeats sequence numbers of their own
    seen, entries, extra = set(), [], list(pk)
    for e in flat:
        si = e[0]
        if 0 <= si < 6 and (si, id(e[1])) in seen:
            extra.append(reseq(pk[si], ssrc, 100 + len(extra)))
            status.append(status[si])
            si = len(extra) - 1
        seen.add((e[0], id(e[1])))
        entries.append((si,) + e[1:4])
    stamps = [stamp(value_of(j), e[4][0], e[4][1]) for j, e in enumerate(flat)]
    f = AstFan(extra, entries, None, stamps, gaps=(16, 48), src_status=status, room=10)
    (seg, ln, st), _ = f.held(e1, "device")
    for j, e in enumerate(flat):
        stamped = e[4][1] and not f.skipped(j)[0] and f.cap[j] >= 24
        assert f.at[j] == (-1 if not stamped else 17 if e[4][0] == 4 else 21), j
        if stamped:
            assert seg[int(f.off[j]) + int(f.at[j]):][:3].tobytes() == value_of(j).to_bytes(3, "big"), j
    if n > 1:
        assert f.n % 2 == 1 and sum(f.skipped(j)[0] for j in range(f.n)) == 6 and (f.at >= 0).sum() == 11
        keep = [j for j in range(f.n) if 0 <= f.src_idx[j] < f.m]
        e2 = make_engine(engine_factory)
        a2, b2 = (Peer([e2], RTP, CM, seed()) for _ in range(2))
        swap = {id(a): a2, id(b): b2}
        g = AstFan(extra, [(entries[j][0], swap[id(entries[j][1])]) + entries[j][2:] for j in keep], None,
                   [stamps[j] for j in keep], src_status=status, room=10)
        g.held(e2, "host")


# ------------------------------------------------------------------ 5. the stride loop
def test_stride_loop(engine_factory, oracle):
    """n = 32768 + 5: only above 32768 entries does a wave take a second pair,
    and both record indices have to move with it.  28-byte sources with the
    element first; every entry has a rewrite record and a stamp record of its
    own (every fifth off, every seventh under the ID of no element)."""
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, CM, seed())
    n = 32768 + 5
    pk = [A.rtp_ext(0x6000 + i, 9, EL, bytes(8)) for i in range(64)]
    assert len(pk[0]) == 28
    entries = [(j % 64, a, 48) for j in range(n)]
    records = [rec(N.REWRITE_SSRC | N.REWRITE_SEQ, 0x00700000 + (j % 4096), 0, 1 + j // 4096) for j in range(n)]
    val = (np.arange(n, dtype=np.uint64) * 2654435761) & 0xFFFFFF
    stamps = [stamp(int(val[j]) | 0x5A000000, 4 if j % 7 == 6 else 3, 0 if j % 5 == 4 else 1, j & 0xFFFF) for j in range(n)]
    f = AstFan(pk, entries, records, stamps)
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert not st.any()
    on = (np.arange(n) % 7 != 6) & (np.arange(n) % 5 != 4)
    assert (f.at == np.where(on, 17, -1)).all()
    b = got[0].reshape(n, 48)[:, 17:20].astype(np.uint64)
    mine = b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]
    assert (mine[on] == val[on]).all() and (mine[~on] == 0xA0A1A2).all()
    assert np.array_equal(f.src_after, f.src_seg)


# --------------------------------------------------------------- 6. with rewrite records
@pytest.mark.parametrize("route", ["host", "device"])
def test_with_rewrite_records(eng, route):
    """All four fields and the stamp: no CSRC and the element first, so the
    setters patch piece 0 and the stamp lies in piece 1 (bytes 17..19), the
    nearest the two can come; the element on the 15/16 boundary of pieces 1/2
    and of pieces 63/64; rewrite records whose mask is 0 beside a stamp;
    and the same entries with no rewrite array at all."""
    peers = [Peer([eng], RTP, CM, seed()) for _ in range(2)]
    ssrc = fresh_ssrc()
    fronts = (0, 9, 14, 15, 63 * 16 + 14 - 17, 63 * 16 + 15 - 17)
    pk = []
    for i, fr in enumerate(fronts):
        body = A.low_words(A.one_byte_ext(A.filler(fr) + [(3, b"\xA0\xA1\xA2"), (7, b"xy")]))
        pk.append(reseq(A.rtp_ext(1, 1, body, bytes(range(50))), ssrc, 20 + i))
    entries = [(i, p) for i in range(len(pk)) for p in peers]
    records = [distinct(j, 0xF if j % 3 else 0) for j in range(len(entries))]
    stamps = [stamp(value_of(j)) for j in range(len(entries))]
    f = AstFan(pk, entries, records, stamps, gaps=(16, 48), room=10)
    (seg, ln, st), _ = f.held(eng, route)
    assert st.tolist() == [0] * f.n
    assert f.at.tolist() == [17 + fr for fr in fronts for _ in peers]
    for j in range(f.n):
        o, si = int(f.off[j]), int(f.src_idx[j])
        hdr = np.frombuffer(pk[si][:12], np.uint8).copy()
        setters(hdr, records[j])
        assert np.array_equal(seg[o:o + 12], hdr), j  # NB: the payload is enciphered, the header is not
        assert seg[o + int(f.at[j]):][:3].tobytes() == value_of(j).to_bytes(3, "big"), j
    # stamp only: rewrite NULL, fresh sequence numbers
    pk2 = [reseq(p, ssrc, 60 + i) for i, p in enumerate(pk)]
    g = AstFan(pk2, entries, None, stamps, gaps=(16, 48), room=10)
    (seg, ln, st), _ = g.held(eng, route)
    assert st.tolist() == [0] * g.n and g.at.tolist() == f.at.tolist()
    for j in range(g.n):
        o, si = int(g.off[j]), int(g.src_idx[j])
        assert seg[o:o + 12].tobytes() == pk2[si][:12] and seg[o + int(g.at[j]):][:3].tobytes() == value_of(j).to_bytes(3, "big")


# ------------------------------------------------------------------------ 7. profiles
def null_peer(engs):
    """NULL cipher, NULL authentication: the copy leaves as it was expanded."""
    pol = SRTPPolicy(0, 0, 0, 0, 0, 0)
    orig = TF.profile_policies
    TF.profile_policies = lambda name: (pol, pol)
    try:
        return Peer(engs, RTP, "NULL_NULL", seed())
    finally:
        TF.profile_policies = orig


@pytest.mark.parametrize("route", ["host", "device"])
def test_profiles(eng, route):
    """One entry each under AES_CM_128_HMAC_SHA1_80, AEAD_AES_128_GCM (the
    stamped bytes are AAD: the tag covers them) and NULL / NULL (the copy leaves
    as it was expanded: the stamp is there in the clear), and an SRTCP
    transformer whose record is off and one whose record is on by mistake (the
    rule knows nothing of the transformer's kind, as for the setters; an RTCP
    packet's first byte has no X bit, so nothing is stamped)."""
    peers = [Peer([eng], RTP, CM, seed()), Peer([eng], RTP, "AEAD_AES_128_GCM", seed()), null_peer([eng])]
    cp = [Peer([eng], RTCP, CM, seed()), Peer([eng], RTCP, CM, seed())]
    ssrc = fresh_ssrc()
    body = A.one_byte_ext([(1, b"z"), (3, b"\xA0\xA1\xA2"), (7, b"pq")])
    pk = [reseq(A.rtp_ext(1, 1, body, bytes(range(40))), ssrc, 30), G.rtcp_packet(ssrc, G.payload(40, 5))]
    entries = [(0, p) for p in peers] + [(1, p) for p in cp]
    stamps = [stamp(value_of(j)) for j in range(3)] + [stamp(0x123456, 3, 0), stamp(0x123456, 3, 1)]
    f = AstFan(pk, entries, None, stamps, gaps=(16, 48), room=24)
    (seg, ln, st), _ = f.held(eng, route)
    assert st.tolist() == [0] * 5 and f.at.tolist() == [19, 19, 19, -1, -1]
    for j in range(3):
        assert seg[int(f.off[j]) + 19:][:3].tobytes() == value_of(j).to_bytes(3, "big")
    o = int(f.off[2])
    assert ln[2] == len(pk[0]) and seg[o:o + len(pk[0])].tobytes() == pk[0][:19] + value_of(2).to_bytes(3, "big") + pk[0][22:]


# ------------------------------------------------- 8. on the device after a receive
def test_forward_on_device_stamped(eng):
    """transform_device(reverse) on the engine's stream, then fanout_device_ast
    on the same stream with that call's length and status tensors as src_len
    and src_status and no synchronise between the two: every peer gets the
    received packets under its own extension ID's element stamped, the dropped
    ones go to nobody."""
    import torch
    snd = Peer([eng], RTP, CM, seed())
    rcv = Peer([eng], RTP, CM, TF._seed[0], sender=False)  # the same keys
    peers = [Peer([eng], RTP, CM, seed()), Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_32", seed())]
    ssrc = fresh_ssrc()
    body = A.one_byte_ext([(4, b"\xB0\xB1\xB2"), (3, b"\xA0\xA1\xA2")])
    clear = [reseq(A.rtp_ext(1, 1, body, G.payload(20 + 9 * (i % 7), i)), ssrc + (i % 4) * 0x100, 100 + i // 4)
             for i in range(32)]
    seg, off, ln, cap = G.pack(clear, room=16)
    assert O.process(snd.r, False, seg, off, ln, cap).tolist() == [0] * 32
    wire = [seg[off[i]:off[i] + ln[i]].tobytes() for i in range(32)]
    b = bytearray(wire[9])
    b[-1] ^= 4  # forged
    wire[9] = bytes(b)
    wire[17] = wire[5]  # replayed
    w_seg, w_off, w_len, w_cap = G.pack(wire, room=0)
    u_seg, u_len = w_seg.copy(), w_len.copy()
    u_st = O.process(rcv.r, True, u_seg, w_off, u_len, w_cap)
    assert sorted(np.nonzero(u_st)[0].tolist()) == [9, 17]
    entries = [(i, p) for i in range(32) for p in peers]
    stamps = [stamp(value_of(2 * i + k), 3 + k) for i in range(32) for k in range(2)]
    f = AstFan(wire, entries, None, stamps, src_len=u_len, src_status=u_st)
    f.src_seg = u_seg  # the sources as the unprotect left them
    ref = f.reference()
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    s = eng.stream_ptr
    r_seg, r_len, r_st = d(w_seg), d(w_len), torch.full((32,), -1, dtype=torch.int32, device="cuda")
    r_off, r_cap = d(w_off), d(w_cap)
    o_seg = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
    o_len = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_st = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_idx, o_tids, o_off, o_cap = d(f.src_idx), d(f.tids), d(f.off), d(f.cap)
    o_ast = torch.from_numpy(f.ast.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    eng.transform_device(True, rcv.tid, r_seg, r_off, r_len, r_cap, r_st, stream=s)
    eng.fanout_device_ast(o_tids, r_seg, r_off, r_len, r_cap, o_idx, o_seg, o_off, o_len, o_cap, o_st, None, o_ast,
                          src_status=r_st, stream=s)
    eng.sync(s)
    torch.cuda.synchronize()
    assert r_st.cpu().numpy().tolist() == u_st.tolist()
    assert np.array_equal(r_seg.cpu().numpy(), u_seg)  # the received bundle is not written by the fan-out
    out = o_seg.cpu().numpy()
    f.check(eng, (out, o_len.cpu().numpy().view(np.uint32), o_st.cpu().numpy()), ref)
    assert (ref[2].reshape(32, 2) == np.where(u_st != 0, 9, 0)[:, None]).all()
    for j in np.nonzero(ref[2] == 0)[0]:
        k = int(j) % 2
        assert f.at[j] == (21, 17)[k] and out[int(f.off[j]) + int(f.at[j]):][:3].tobytes() == value_of(int(j)).to_bytes(3, "big")


# ------------------------------------------------- 9. nothing changes without records
@pytest.mark.parametrize("route", ["host", "device"])
def test_nothing_changes_without_records(engine_factory, oracle, route):
    """stamp=None against fanout_*_rw on an identical engine, with rewrite
    records and without: statuses, lengths, the destination bytes (device: the
    whole segment bit for bit; host: every OK region) and fanout_stats."""
    engs = [make_engine(engine_factory) for _ in range(2)]
    peers = [Peer(engs, RTP, name, seed()) for name in (CM, "F8_128_HMAC_SHA1_80", CM)]
    ssrc = fresh_ssrc()
    pk = [reseq(A.rtp_ext(1, 1, EL, G.payload(20 + 37 * i, i)), ssrc + (i << 8), 40 + i) for i in range(7)] + [b"\x80" * 8]
    entries = [(i, p) for i in range(len(pk)) for p in peers]
    for rewritten in (True, False):
        records = [distinct(j, (5 * j + 3) % 16) for j in range(len(entries))] if rewritten else None
        f = AstFan([reseq(p, ssrc + (i << 8), 40 + 50 * rewritten + i) for i, p in enumerate(pk)], entries, records,
                   [stamp(value_of(j)) for j in range(len(entries))], gaps=(16,), room=10)
        f.pass_stamps = False
        got = f.run(engs[0], route)
        rw = RwFan(f.pkts, entries, records or [rec()] * f.n, gaps=(16,), room=10)
        rw.pass_records = rewritten
        want = rw.run_host(engs[1]) if route == "host" else rw.run_device(engs[1])
        rw.check(engs[1], want, which=1)
        assert got[2].tolist() == want[2].tolist() and got[1].tolist() == want[1].tolist()
        if route == "device":
            assert np.array_equal(got[0], want[0])
        for j in np.nonzero(want[2] == 0)[0]:
            o = int(f.off[j])
            assert np.array_equal(got[0][o:o + int(want[1][j])], want[0][o:o + int(want[1][j])]), j
        assert engs[0].fanout_stats() == engs[1].fanout_stats()


# ------------------------------------------------------------------ 10. argument rules
def test_argument_rules(engine_factory, oracle):
    """A device array misaligned by 4 bytes is SRTP_EINVAL with nothing
    launched: the output arrays as they were, no context made, the statistics
    unmoved.  Aligned, the same call goes through."""
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, CM, seed())
    ssrc = fresh_ssrc()
    pk = [reseq(A.rtp_ext(1, 1, EL, bytes(24)), ssrc, 4 + i) for i in range(3)]
    f = AstFan(pk, [(i, a) for i in range(3)], None, [stamp(value_of(j)) for j in range(3)])
    st0 = e1.fanout_stats()
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        f.run_device(e1, misalign=4)
    assert (f.seg_after == FILL).all() and np.array_equal(f.src_after, f.src_seg)
    assert e1.fanout_stats() == st0 and e1.context_state(a.e[0], ssrc) is None
    (seg, ln, st), _ = f.held(e1, "device")
    assert st.tolist() == [0, 0, 0] and f.at.tolist() == [17] * 3
    assert e1.fanout_stats()["calls"] == st0["calls"] + 1


# ------------------------------------------------------------------------ 11. fan_out_ast()
class Clock:
    """A stateful stamper: every call reads a clock that has moved on 1.5 ms, as
    AbsSendTimeEngine reads System.nanoTime() for every packet it sends."""

    def __init__(self, ext_id, start_ns):
        self.ext_id, self.ns, self.calls = ext_id, start_ns, 0

    def __call__(self, pkt):
        self.ns += 1500000
        self.calls += 1
        return self.ext_id, abs_send_time(self.ns)


def test_fan_out_ast_api(engine_factory, oracle):
    """fan_out_ast against fan_out_rw, on a twin engine, of packets stamped on
    the host by the restatement in doWrite's order.  One stamper is shared by
    two transformers and stateful, one returns None for every second packet,
    one transformer has no stamper; one transformer also has a rewriter."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    peers = [Peer([e1, e2], RTP, name, seed()) for name in (CM, "AEAD_AES_256_GCM", CM, "F8_128_HMAC_SHA1_80")]
    ssrc = fresh_ssrc()
    body = A.one_byte_ext([(4, b"\xB0\xB1\xB2"), (3, b"\xA0\xA1\xA2")])
    raw = [reseq(A.rtp_ext(1, 1, body, G.payload(30 + 13 * i, i)), ssrc, 30 + i) for i in range(5)]
    pkts = [RawPacket(b"\x00" * 3 + r, 3, len(r)) if i != 2 else None for i, r in enumerate(raw)]
    before = [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts]
    shared, start = Clock(3, 63 * 10 ** 9 + 999000000), 63 * 10 ** 9 + 999000000
    flip = [0]

    def every_second(pkt):
        flip[0] += 1
        return (4, 0xABCDEF) if flip[0] & 1 else None
    rewriter = lambda pkt: {"pt": 111}
    out = fan_out_ast(pkts, [p.e[0] for p in peers], [None, None, rewriter, None], [shared, shared, every_second, None])
    assert [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts] == before
    assert len(out) == 4 and shared.calls == 8
    # the host's way: stamp host-made copies in doWrite's order, then fan_out_rw without stampers
    model, flip2 = Clock(3, start), 0
    copies = [[None] * 5 for _ in peers]
    for i, r in enumerate(raw):
        if pkts[i] is None:
            continue
        for k in range(4):
            buf = bytearray(r)
            if k < 2:
                ext_id, value = model(None)
                assert A.stamp(buf, ext_id, value) == 21
            elif k == 2:
                flip2 += 1
                if flip2 & 1:
                    assert A.stamp(buf, 4, 0xABCDEF) == 17
            copies[k][i] = RawPacket(bytes(buf), 0, len(buf))
    assert abs_send_time(start + 1500000) < abs_send_time(start)  # the 6-bit seconds wrapped on the way
    for k, p in enumerate(peers):
        want = fan_out_rw(copies[k], [p.e[1]], [rewriter if k == 2 else None])[0]
        for i in range(5):
            assert (out[k][i] is None) == (want[i] is None) == (i == 2), (k, i)
            if want[i] is not None:
                assert out[k][i].data() == want[i].data(), (k, i)
    got, ref = e1.context_state(peers[0].e[0], ssrc), e2.context_state(peers[0].e[1], ssrc)
    for key in KEYS_RTP:
        assert got[key] == ref[key]
