"""Fan-out that patches the payload per destination (srtp_fanout_device_pay /
_host_pay, k_fanout_pay, fan_out_pay()): each destination entry carries an
8-byte record of two patches (at0, b0[2], at1, b1[2]) -- the RTX original
sequence number and the FEC header's SN base, which
ExtendedSequenceNumberInterval.rewriteRTP writes per peer -- written into the
copy before the protect chain runs.

The expected result is built as for the other fan-out tests: the entries are
expanded on the host with numpy, each host-made copy gets RawPacket's four
setters where a rewrite record is present, then the reference's payload writes
(payload_ref: patch 0, patch 1, per byte under the bound), then
AbsSendTimeEngine's stamp (abs_send_time_ref, over the bytes as patched), and
that bundle goes through the references (oracle.process, gcm_ref.process).
Equal ciphertext and tags show that the bytes stood before the cipher ran."""
import numpy as np
import pytest

import abs_send_time_ref as A
import gcm_ref as G
import payload_ref as P
from libjitsi_amd import RawPacket, fan_out_ast, fan_out_pay, fec_sn_bytes
from libjitsi_amd import _native as N
from oracle import oracle as O
from test_fanout import FILL, KEYS_RTP, RTP, SKIP, Peer, make_engine, rtp, seed, up16
from test_fanout_ast import AstFan, reseq, stamp, value_of
from test_fanout_rewrite import RwFan, distinct, rec, setters
import test_fanout as TF

pytestmark = pytest.mark.gpu

CM = "AES_CM_128_HMAC_SHA1_80"
INVALID = N.STATUS_DROP_INVALID
OFF = stamp(0, 3, 0)


def pay(at0=0, b0=(0, 0), at1=0, b1=(0, 0)):
    return (at0, tuple(b0), at1, tuple(b1))


def bytes_of(j, k=0):
    """Two bytes that change with j (and differ between the two patches), none equal to FILL."""
    a, b = (0x11 + 5 * j + 0x40 * k) & 0xFF, (0x83 + 11 * j + 0x20 * k) & 0xFF
    return (a if a != FILL else 1, b if b != FILL else 2)


class PayFan(AstFan):
    """AstFan with one payload record per entry.  stamps None: no stamp array
    is passed; pays None: no payload array is passed (the _ast call)."""

    def __init__(self, pkts, entries, records, stamps, pays, **kw):
        super().__init__(pkts, entries, records, stamps if stamps is not None else [OFF] * len(entries), **kw)
        self.pass_stamps = stamps is not None
        self.pass_pays = pays is not None
        pays = pays if pays is not None else [pay()] * self.n
        assert len(pays) == self.n
        self.py = np.array([tuple(p) for p in pays], N.FANOUT_PAYLOAD_DTYPE).reshape(self.n)

    def expand(self, rounded=False):
        seg, ln, fl = RwFan.expand(self, rounded)  # the setters
        for j in range(self.n):
            c = self.copied(j)
            if c <= 0:
                continue
            o = int(self.off[j])
            buf = bytearray(seg[o:o + c].tobytes())
            if self.pass_pays:
                P.apply(buf, self.py[j])
            if c >= 12 and self.pass_stamps:
                self.at[j] = A.apply(buf, self.ast[j])
            seg[o:o + c] = np.frombuffer(bytes(buf), np.uint8)
        return seg, ln, fl

    def pays(self):
        return self.py if self.pass_pays else None

    def run_host(self, eng):
        seg = np.full(self.seg_bytes, FILL, np.uint8)
        src = self.src_seg.copy()
        ln, st = eng.fanout_host_pay(self.tids, self.src_seg, self.src_off, self.src_len, self.src_cap, self.src_idx,
                                     seg, self.off, self.cap, self.src_status,
                                     self.flags if self.flags.any() else None, self.records(), self.stamps(),
                                     self.pays())
        assert np.array_equal(src, self.src_seg)
        return seg, ln, st

    def run_device(self, eng, stream=None, misalign=0):
        import torch
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

        def records(arr, size):
            if arr is None:
                return None
            raw = torch.zeros(size * self.n + 16, dtype=torch.uint8, device="cuda")
            raw[:size * self.n].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()))
            return raw[:size * self.n]
        src_seg = d(self.src_seg)
        seg = torch.full((self.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        args = [d(self.src_off), d(self.src_len), d(self.src_cap), d(self.src_idx), seg, d(self.off), ln, d(self.cap), st]
        rw, ast = records(self.records(), 16), records(self.stamps(), 8)
        py = None
        if self.pays() is not None:
            raw = torch.zeros(8 * self.n + 16, dtype=torch.uint8, device="cuda")
            py = raw[misalign:misalign + 8 * self.n]
            py.copy_(torch.from_numpy(self.py.view(np.uint8).reshape(-1).copy()))
        src_status = None if self.src_status is None else d(self.src_status)
        flags = d(self.flags) if self.flags.any() else None
        torch.cuda.synchronize()
        try:
            eng.fanout_device_pay(d(self.tids), src_seg, *args, rw, ast, py, src_status=src_status, flags=flags,
                                  stream=stream)
        finally:
            eng.sync(stream)
            torch.cuda.synchronize()
            self.src_after = src_seg.cpu().numpy()
            self.seg_after = seg.cpu().numpy()
        return self.seg_after, ln.cpu().numpy().view(np.uint32), st.cpu().numpy()


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


_ssrc = [0x0B570000]


def fresh_ssrc():
    _ssrc[0] += 0x100
    return _ssrc[0]


# ------------------------------------------------------------------ 1. the positions
@pytest.mark.parametrize("route", ["host", "device"])
def test_positions(eng, route):
    """One source of 2080 bytes (c = 2080: 130 pieces, the second trip holds
    pieces 128 and 129), every entry toward a peer of its own: a patch at byte
    12 beside all four setters, at 11 (refused), around the piece boundary at
    32, around 1024 (lane 63's first piece against lane 0's second), around 2048
    (the first trip against the second), at c - 2, c - 1 (one byte written), c
    and c + 1; both patches in one piece and in one word; equal offsets and
    offsets one apart, both ways round (patch 1 wins); patch 1 alone; and
    destinations of 1000 bytes that truncate below the offset, at it, and one
    byte behind it (those end DROP_INVALID: on the device route the copy is
    held to the expanded bytes up to up16(cap), and FILL behind)."""
    ssrc = fresh_ssrc()
    src = [rtp(ssrc, 77, 2080)]
    c = 2080
    one = [12, 11, 30, 31, 32, 1022, 1023, 1024, 2046, 2047, 2048, c - 2, c - 1, c, c + 1]
    two = [(40, 44), (52, 53), (100, 100), (100, 101), (101, 100), (0, 1023), (2047, 31), (c - 1, c - 2)]
    cut = [(1500, 0), (999, 998), (1000, 999), (1001, 12)]
    pays = [pay(a, bytes_of(j)) for j, a in enumerate(one)]
    pays += [pay(a, bytes_of(j), b, bytes_of(j, 1)) for j, (a, b) in enumerate(two)]
    pays += [pay(a, bytes_of(j), b, bytes_of(j, 1)) for j, (a, b) in enumerate(cut)]
    n = len(pays)
    peers = [Peer([eng], RTP, CM, seed()) for _ in range(n)]
    entries = [(0, p) if j < n - len(cut) else (0, p, 1000) for j, p in enumerate(peers)]
    records = [distinct(0, 0xF)] + [rec()] * (n - 1)
    f = PayFan(src, entries, records, None, pays, gaps=(16, 48), room=10)
    (seg, ln, st), _ = f.held(eng, route)
    assert st.tolist() == [0] * (n - len(cut)) + [INVALID] * len(cut) and n == 27
    # the reference itself did what the docstring says
    exp = f.expand()[0]
    plain = np.frombuffer(src[0], np.uint8)
    changed = [np.nonzero(exp[int(f.off[j]):][:f.copied(j)][12:] != plain[12:f.copied(j)])[0] + 12 for j in range(n)]
    assert changed[0].tolist() == [12, 13] and changed[1].size == 0
    assert changed[12].tolist() == [c - 1] and changed[13].size == 0 and changed[14].size == 0
    assert changed[17].tolist() == [100, 101] and exp[int(f.off[17]) + 100] == bytes_of(2, 1)[0]
    assert exp[int(f.off[18]) + 100:][:3].tolist() == [bytes_of(3)[0], bytes_of(3, 1)[0], bytes_of(3, 1)[1]]
    assert changed[n - 4].size == 0 and changed[n - 3].tolist() == [998, 999] and changed[n - 2].tolist() == [999]


# -------------------------------------------------------------------- 2. the pairs
@pytest.mark.parametrize("n", [21, 1])
def test_pairs(engine_factory, oracle, n):
    """Wave pairs (entries 2k, 2k + 1): one entry skipped by its flag, by its
    index and by its source's status, one whose region holds no byte and one of
    8 bytes, each beside a partner with bytes, both ways round, each with a
    live record of its own at another offset than its partner's; an odd number
    of entries, and a single one.  A skipped entry's region stays FILL; the
    partner is patched by its own record only (held() compares every byte of
    the regions).  Device route (the host route refuses an index that names no
    source); then the host route without that pair."""
    e1 = make_engine(engine_factory)
    a, b = (Peer([e1], RTP, CM, seed()) for _ in range(2))
    ssrc = fresh_ssrc()
    pk = [rtp(ssrc, 10 + i, L) for i, L in enumerate((28, 100, 33, 1200, 64, 40))]
    status = [0, 0, 0, 0, 0, N.STATUS_DROP_AUTH]
    K = SKIP
    # (source, peer, cap, flags, at0)
    pairs = [((0, a, None, 0, 12), (0, b, None, 0, 20)), ((1, a, None, 0, 15), (1, b, None, 0, 0)),
             ((2, a, None, 0, 0), (2, b, None, 0, 31)), ((3, a, None, 0, 1023), (3, b, None, K, 1023)),
             ((4, a, None, K, 20), (4, b, None, 0, 47)), ((5, a, None, 0, 14), (0, a, None, 0, 26)),
             ((1, a, None, 0, 63), (5, b, None, 0, 12)), ((2, a, None, 0, 16), (1000, b, 64, 0, 16)),
             ((-1, a, 64, 0, 13), (3, a, None, 0, 1199)), ((4, a, None, 0, 62), (1, b, 0, 0, 62)),
             ((2, b, 8, 0, 12), (3, b, None, 0, 12))]
    flat = [e for pr in pairs for e in pr][:n] if n > 1 else [pairs[0][1]]
    seen, entries, extra = set(), [], list(pk)
    for e in flat:
        si = e[0]
        if 0 <= si < 6 and (si, id(e[1])) in seen:  # a repeat toward one peer: a sequence number of its own
            extra.append(reseq(pk[si], ssrc, 100 + len(extra)))
            status.append(status[si])
            si = len(extra) - 1
        seen.add((e[0], id(e[1])))
        entries.append((si,) + e[1:4])
    pays = [pay(e[4], bytes_of(j), e[4] + 3 if e[4] else 0, bytes_of(j, 1)) for j, e in enumerate(flat)]
    f = PayFan(extra, entries, None, None, pays, gaps=(16, 48), src_status=status, room=10)
    (seg, ln, st), _ = f.held(e1, "device")
    exp = f.expand()[0]
    for j, e in enumerate(flat):
        o, live = int(f.off[j]), e[4] and not f.skipped(j)[0] and f.cap[j] > e[4]
        if live:  # each byte below c is its own record's
            want = {e[4]: bytes_of(j)[0], e[4] + 1: bytes_of(j)[1], e[4] + 3: bytes_of(j, 1)[0], e[4] + 4: bytes_of(j, 1)[1]}
            assert all(exp[o + i] == v for i, v in want.items() if i < f.copied(j)), j
        if f.skipped(j)[0]:
            assert (seg[o:o + up16(f.cap[j])] == FILL).all(), j
    if n > 1:
        assert f.n % 2 == 1 and sum(f.skipped(j)[0] for j in range(f.n)) == 6
        keep = [j for j in range(f.n) if 0 <= f.src_idx[j] < f.m]
        e2 = make_engine(engine_factory)
        a2, b2 = (Peer([e2], RTP, CM, seed()) for _ in range(2))
        swap = {id(a): a2, id(b): b2}
        g = PayFan(extra, [(entries[j][0], swap[id(entries[j][1])]) + entries[j][2:] for j in keep], None, None,
                   [pays[j] for j in keep], src_status=status, room=10)
        g.held(e2, "host")


# ------------------------------------------------------------------ 3. the stride loop
def test_stride_loop(engine_factory, oracle):
    """n = 32768 + 5: only above 32768 entries does a wave take a second pair,
    and the record index has to move with it.  64-byte sources; every entry has
    a rewrite record (an SSRC and sequence number of its own) and a payload
    record derived from j: both offsets and all four bytes.  Every entry goes
    through the reference; the first and last entries of each stride and a
    sample are also read back in the clear through a NULL-cipher peer."""
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, "NULL_HMAC_SHA1_80", seed())
    n = 32768 + 5
    pk = [rtp(0x6100 + i, 9, 64) for i in range(64)]
    entries = [(j % 64, a, 80) for j in range(n)]
    records = [rec(N.REWRITE_SSRC | N.REWRITE_SEQ, 0x00710000 + (j % 4096), 0, 1 + j // 4096) for j in range(n)]
    jj = np.arange(n)
    at0, at1 = 12 + jj % 51, 12 + (7 * jj + 3) % 52
    pays = [pay(int(at0[j]), (j & 0xFF, (j >> 8) & 0xFF), int(at1[j]), ((j >> 3) & 0xFF, (j * 13) & 0xFF)) for j in range(n)]
    f = PayFan(pk, entries, records, None, pays)
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert not st.any()
    out = got[0].reshape(n, 80)
    for j in sorted({0, 1, 32766, 32767, 32768, 32769, n - 2, n - 1} | set(range(5, n, 997))):
        want = bytearray(pk[j % 64])
        P.apply(want, pays[j])
        assert out[j, 12:64].tobytes() == bytes(want[12:]), j  # NULL cipher: the payload in the clear
    assert np.array_equal(f.src_after, f.src_seg)


# ------------------------------------------------------ 4. with rewrite and stamp records
EL = b"\x32\xA0\xA1\xA2"  # ID 3, len field 2


@pytest.mark.parametrize("route", ["host", "device"])
def test_with_rewrite_and_stamp(eng, route):
    """All three kinds of record on in every entry; then each kind alone through
    _pay with the other arrays NULL.  Sources: the element in the usual place
    with the OSN at the payload's first byte; the element on the 15/16 boundary
    of pieces 1/2 with a patch in the same piece; and test_fanout_ast's
    stamp-quirk packet, whose walk steps four bytes past the extension and
    matches in the payload: the stamp lands on payload bytes 1..3, over the
    OSN's second byte.  There the stamp's bytes win and the OSN's first byte
    stands -- and since the reference walks the copy the rewriting engine has
    written, an OSN whose first byte reads as another element decides whether
    the copy is stamped at all: 0x32.. (ID 3) and 0x42.. (ID 4, which the source
    does not carry) are stamped under those IDs, 0x52.. under ID 3 is not."""
    peers = [Peer([eng], RTP, CM, seed()) for _ in range(3)]
    ssrc = fresh_ssrc()
    body = A.low_words(A.one_byte_ext(A.filler(14) + [(3, b"\xA0\xA1\xA2"), (7, b"xy")]))
    shapes = [A.rtp_ext(1, 1, EL, bytes(range(50))), A.rtp_ext(1, 1, body, bytes(range(50))),
              A.rtp_ext(1, 1, bytes(4), EL + bytes(range(40)), words=1)]
    hl = [RawPacket(p, 0, len(p)).getHeaderLength() for p in shapes]
    assert hl[2] == 20 and shapes[2][20:24] == EL

    def run(base, use_rw, use_ast, use_pay):
        pk = [reseq(p, ssrc + i, base + i) for i, p in enumerate(shapes)]
        entries = [(i, p) for i in range(3) for p in peers]
        osn = [0x32C7, 0x42C8, 0x52C9]
        ids = [3, 4, 3]
        pays = [pay(hl[i] + 6, bytes_of(3 * i + k), hl[i], (osn[k] >> 8, osn[k] & 0xFF)) for i in range(3) for k in range(3)]
        stamps = [stamp(value_of(3 * i + k), ids[k] if i == 2 else 3) for i in range(3) for k in range(3)]
        records = [distinct(base + j, 0xF if j % 4 else 0) for j in range(9)]
        f = PayFan(pk, entries, records if use_rw else None, stamps if use_ast else None, pays if use_pay else None,
                   gaps=(16, 48), room=10)
        (seg, ln, st), _ = f.held(eng, route)
        assert st.tolist() == [0] * 9
        return f, seg

    f, seg = run(20, True, True, True)
    assert f.at.tolist() == [17, 17, 17, 31, 31, 31, 21, 21, -1]
    exp = f.expand()[0]
    for k, first in enumerate((0x32, 0x42, 0x52)):
        o = int(f.off[6 + k])
        assert exp[o + 20] == first  # the OSN's first byte stands
        if k < 2:
            assert exp[o + 21:o + 24].tobytes() == value_of(6 + k).to_bytes(3, "big")  # the stamp won byte 21
        else:
            assert exp[o + 21] == 0xC9 and exp[o + 22:o + 24].tobytes() == EL[2:]
    f, _ = run(40, False, False, True)
    assert (f.at == -1).all()
    f, _ = run(60, False, True, False)
    assert f.at.tolist() == [17, 17, 17, 31, 31, 31, 21, -1, 21]  # the source's own element: ID 3
    f, _ = run(80, True, False, False)
    f, _ = run(100, True, False, True)
    f, _ = run(120, False, True, True)
    assert f.at.tolist() == [17, 17, 17, 31, 31, 31, 21, 21, -1]


# ------------------------------------------------------------------------ 5. profiles
@pytest.mark.parametrize("route", ["host", "device"])
def test_profiles(eng, route):
    """AES_CM_128_HMAC_SHA1_80, AEAD_AES_128_GCM, the NULL cipher with HMAC and
    an F8 peer in one bundle, two sources each, both patches on: equal
    ciphertext and tags show that the patch stood before the cipher and the
    seal; under the NULL cipher the bytes are there in the clear."""
    names = (CM, "AEAD_AES_128_GCM", "NULL_HMAC_SHA1_80", "F8_128_HMAC_SHA1_80")
    peers = [Peer([eng], RTP, name, seed()) for name in names]
    ssrc = fresh_ssrc()
    pk = [rtp(ssrc, 30, 200), rtp(ssrc + 1, 31, 47)]
    entries = [(i, p) for i in range(2) for p in peers]
    pays = [pay(12, bytes_of(j), 45 if i else 143, bytes_of(j, 1)) for j, (i, _) in enumerate(entries)]
    f = PayFan(pk, entries, None, None, pays, gaps=(16, 48), room=24)
    (seg, ln, st), ref = f.held(eng, route)
    assert st.tolist() == [0] * 8
    for j in (2, 6):
        o, i = int(f.off[j]), j // 4
        want = P.apply(bytearray(pk[i]), pays[j])
        assert bytes(want) != pk[i] and seg[o:o + len(pk[i])].tobytes() == bytes(want)
    plain = PayFan([reseq(p, ssrc + 16 + i, 30) for i, p in enumerate(pk)], entries, None, None, None, gaps=(16, 48),
                   room=24)
    seg0 = plain.reference()[0]
    for j in range(8):  # the patched plaintext changed what the cipher and the tag made of it
        o, L = int(f.off[j]), int(ref[1][j])
        assert not np.array_equal(ref[0][o + 12:o + L], seg0[o + 12:o + L]), j


# ---------------------------------------------------------------------- 6. an RTX stream
def test_rtx_stream(engine_factory, oracle):
    """Packets of an RTX SSRC toward two peers, each under the peer's target
    RTX SSRC with the peer's sequence numbers -- across the wrap at 65535 --
    and the peer's OSN in the payload's first two bytes.  The sender's context
    exists under the target SSRC with ROC 1 and none under the source's; each
    peer's receiver unprotects every copy and finds the expected OSN."""
    e1 = make_engine(engine_factory)
    snd, rcv = [], []
    for _ in range(2):
        s = seed()
        snd.append(Peer([e1], RTP, CM, s))
        rcv.append(Peer([e1], RTP, CM, s, sender=False))
    src_ssrc = fresh_ssrc()
    target = [src_ssrc + 0x10, src_ssrc + 0x20]
    pk = [G.rtp_packet(src_ssrc, 500 + i, (0x7000 + i).to_bytes(2, "big") + G.payload(40 + 7 * i, i)) for i in range(6)]
    seq = lambda k, i: (65533 + 2 * k + i) & 0xFFFF
    osn = lambda k, i: (65531 + 300 * k + i) & 0xFFFF
    entries = [(i, snd[k]) for i in range(6) for k in range(2)]
    records = [rec(N.REWRITE_SSRC | N.REWRITE_SEQ, target[k], 0, seq(k, i)) for i in range(6) for k in range(2)]
    pays = [pay(0, (0, 0), 12, (osn(k, i) >> 8, osn(k, i) & 0xFF)) for i in range(6) for k in range(2)]
    f = PayFan(pk, entries, records, None, pays, room=10)
    (seg, ln, st), _ = f.held(e1, "device")
    assert st.tolist() == [0] * 12
    for k in range(2):
        state = e1.context_state(snd[k].e[0], target[k])
        assert state is not None and state["roc"] == 1
        assert e1.context_state(snd[k].e[0], src_ssrc) is None
    back, ln2 = seg.copy(), ln.copy()
    tids = np.array([rcv[k].tid for _ in range(6) for k in range(2)], np.int32)
    st2 = e1.transform_host(True, tids, back, f.off, ln2, f.cap)
    assert st2.tolist() == [0] * 12
    for j in range(12):
        i, k = divmod(j, 2)
        p = back[int(f.off[j]):][:int(ln2[j])].tobytes()
        assert len(p) == len(pk[i])
        assert int.from_bytes(p[8:12], "big") == target[k] and int.from_bytes(p[2:4], "big") == seq(k, i)
        assert int.from_bytes(p[12:14], "big") == osn(k, i) and p[14:] == pk[i][14:], j


# ------------------------------------------------- 7. nothing changes without records
@pytest.mark.parametrize("route", ["host", "device"])
def test_nothing_changes_without_records(engine_factory, oracle, route):
    """pay=None against fanout_*_ast on an identical engine, with stamp and
    rewrite records: statuses, lengths, the destination bytes (device: the whole
    segment bit for bit; host: every OK region) and fanout_stats."""
    engs = [make_engine(engine_factory) for _ in range(2)]
    peers = [Peer(engs, RTP, name, seed()) for name in (CM, "F8_128_HMAC_SHA1_80", CM)]
    ssrc = fresh_ssrc()
    pk = [reseq(A.rtp_ext(1, 1, EL, G.payload(20 + 37 * i, i)), ssrc + i, 40 + i) for i in range(7)] + [b"\x80" * 8]
    entries = [(i, p) for i in range(len(pk)) for p in peers]
    for with_records in (True, False):
        records = [distinct(j, (5 * j + 3) % 16) for j in range(len(entries))] if with_records else None
        stamps = [stamp(value_of(j)) for j in range(len(entries))] if with_records else None
        src = [reseq(p, ssrc + i, 40 + 50 * with_records + i) for i, p in enumerate(pk)]
        f = PayFan(src, entries, records, stamps, None, gaps=(16,), room=10)
        got = f.run(engs[0], route)
        if with_records:
            old = AstFan(src, entries, records, stamps, gaps=(16,), room=10)
        else:
            old = RwFan(src, entries, [rec()] * f.n, gaps=(16,), room=10)
            old.pass_records = False
        want = old.run_host(engs[1]) if route == "host" else old.run_device(engs[1])
        old.check(engs[1], want, which=1)
        assert got[2].tolist() == want[2].tolist() and got[1].tolist() == want[1].tolist()
        if route == "device":
            assert np.array_equal(got[0], want[0])
        for j in np.nonzero(want[2] == 0)[0]:
            o = int(f.off[j])
            assert np.array_equal(got[0][o:o + int(want[1][j])], want[0][o:o + int(want[1][j])]), j
        assert engs[0].fanout_stats() == engs[1].fanout_stats()


# ------------------------------------------------------------------ 8. argument rules
def test_argument_rules(engine_factory, oracle):
    """A device array misaligned by 4 bytes is SRTP_EINVAL with nothing
    launched: the output arrays as they were, no context made, the statistics
    unmoved.  Aligned, the same call goes through.  Fewer than n records are a
    ValueError in Python, on both routes, before any call."""
    import torch
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, CM, seed())
    ssrc = fresh_ssrc()
    pk = [rtp(ssrc, 4 + i, 60) for i in range(3)]
    f = PayFan(pk, [(i, a) for i in range(3)], None, None, [pay(12, bytes_of(j)) for j in range(3)])
    st0 = e1.fanout_stats()
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        f.run_device(e1, misalign=4)
    assert (f.seg_after == FILL).all() and np.array_equal(f.src_after, f.src_seg)
    assert e1.fanout_stats() == st0 and e1.context_state(a.e[0], ssrc) is None
    seg = np.full(f.seg_bytes, FILL, np.uint8)
    with pytest.raises(ValueError):
        e1.fanout_host_pay(f.tids, f.src_seg, f.src_off, f.src_len, f.src_cap, f.src_idx, seg, f.off, f.cap,
                           pay=f.py[:2])
    d = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()
    out = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
    ln, st = (torch.full((3,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    short = torch.zeros(8 * 3 - 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        e1.fanout_device_pay(d(f.tids), d(f.src_seg), d(f.src_off), d(f.src_len), d(f.src_cap), d(f.src_idx), out,
                             d(f.off), ln, d(f.cap), st, None, None, short)
    torch.cuda.synchronize()
    assert (seg == FILL).all() and (out.cpu().numpy() == FILL).all() and e1.fanout_stats() == st0
    (seg, ln, st), _ = f.held(e1, "device")
    assert st.tolist() == [0, 0, 0]
    assert e1.fanout_stats()["calls"] == st0["calls"] + 1


# ------------------------------------------------------------------------ 9. fan_out_pay()
def test_fan_out_pay_api(engine_factory, oracle):
    """fan_out_pay against fan_out_ast, on a twin engine, of packets patched on
    the host by the restatement: one transformer's rewriter returns osn, one
    fec, one both (with pt, and a stamper behind it), one has no rewriter.  An
    FEC offset or a header length outside 12 .. 65535 - 2 is a ValueError, and
    fan_out_ast and fan_out_rw keep refusing the two keys."""
    from libjitsi_amd import fan_out_rw
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    peers = [Peer([e1, e2], RTP, name, seed()) for name in (CM, "AEAD_AES_256_GCM", CM, "F8_128_HMAC_SHA1_80")]
    ssrc = fresh_ssrc()
    body = A.one_byte_ext([(4, b"\xB0\xB1\xB2"), (3, b"\xA0\xA1\xA2")])
    raw = [reseq(A.rtp_ext(1, 1, body, G.payload(40 + 13 * i, i)), ssrc, 30 + i) for i in range(4)]
    raw.append(rtp(ssrc, 34, 60))  # no extension: the payload starts at byte 12
    pkts = [RawPacket(b"\x00" * 3 + r, 3, len(r)) if i != 2 else None for i, r in enumerate(raw)]
    before = [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts]
    count = [0]

    def osn_of(pkt):
        count[0] += 1
        return {"osn": 0xFFF0 + count[0]}
    fec_of = lambda pkt: {"fec": (pkt.getHeaderLength() + 5, 0x1234)}
    both = lambda pkt: {"pt": 111, "osn": 0xBEEF, "fec": (pkt.getHeaderLength() + 2, 0xABCD)}
    stamper = lambda pkt: (3, 0x123456)
    out = fan_out_pay(pkts, [p.e[0] for p in peers], [osn_of, fec_of, both, None], [None, None, stamper, None])
    assert [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts] == before
    assert len(out) == 4 and count[0] == 4
    copies, calls = [[None] * 5 for _ in peers], 0
    for i, r in enumerate(raw):
        if pkts[i] is None:
            continue
        h = pkts[i].getHeaderLength()
        assert h == (24 if i < 4 else 12)
        for k in range(4):
            buf = bytearray(r)
            if k == 0:
                calls += 1
                P.write_short(buf, h, 0xFFF0 + calls)
            elif k == 1:
                P.rewrite_fec(buf, h + 5, 0x1234)
                assert bytes(buf[h + 7:h + 9]) == b"\x34\x34"
            elif k == 2:
                P.rewrite_fec(buf, h + 2, 0xABCD)  # rewriteRTP's order: the FEC store, then the OSN
                P.write_short(buf, h, 0xBEEF)
            assert (bytes(buf) != r) == (k < 3)
            copies[k][i] = RawPacket(bytes(buf), 0, len(buf))
    for k, p in enumerate(peers):
        want = fan_out_ast(copies[k], [p.e[1]], [(lambda pkt: {"pt": 111}) if k == 2 else None],
                           [stamper if k == 2 else None])[0]
        for i in range(5):
            assert (out[k][i] is None) == (want[i] is None) == (i == 2), (k, i)
            if want[i] is not None:
                assert out[k][i].data() == want[i].data(), (k, i)
    got, ref = e1.context_state(peers[0].e[0], ssrc), e2.context_state(peers[0].e[1], ssrc)
    for key in KEYS_RTP:
        assert got[key] == ref[key]
    one, t = [pkts[0]], [peers[0].e[0]]
    for bad in ({"fec": (11, 1)}, {"fec": (65534, 1)}, {"fec": (-1, 1)}, {"nack": 1}):
        with pytest.raises(ValueError):
            fan_out_pay(one, t, [lambda pkt: bad], [None])
    for key in ({"osn": 1}, {"fec": (20, 1)}):
        with pytest.raises(ValueError):
            fan_out_ast(one, t, [lambda pkt: key], [None])
        with pytest.raises(ValueError):
            fan_out_rw(one, t, [lambda pkt: key])
    assert fec_sn_bytes(0x1234) == (0x34, 0x34)
