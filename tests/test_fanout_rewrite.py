"""Fan-out with per-destination rewriting (srtp_fanout_device_rw / _host_rw,
k_fanout_rw, fan_out_rw()): each destination entry carries a record with the
target SSRC, sequence number, timestamp and payload type of its peer's send
chain, written into the copy on the device before the protect chain parses it.

The expected result is built as for fan-out: the entries are expanded on the
host with numpy, RawPacket's four setters are applied byte by byte to every
host-made copy of at least 12 bytes whose record names a field, and that bundle
goes through the references (oracle.process, gcm_ref.process).  Compared:
status and length of every entry, the bytes [off, off + len) of every OK entry,
and the state of every (transformer, SSRC) context, read under the rewritten
SSRC and under the source's."""
import numpy as np
import pytest

import gcm_ref as G
from libjitsi_amd import RawPacket, fan_out_rw
from libjitsi_amd import _native as N
from oracle import oracle as O
from test_fanout import (FILL, KEYS_RTCP, KEYS_RTP, RTCP, RTCP_PROFILES, RTP, RTP_PROFILES, SKIP, Fan, Peer,
                         make_engine, profile_fan, rtp, seed, twin_equal, up16)
import test_fanout as TF

pytestmark = pytest.mark.gpu

SSRC, SEQ, TS, PT = N.REWRITE_SSRC, N.REWRITE_SEQ, N.REWRITE_TIMESTAMP, N.REWRITE_PT
CM = "AES_CM_128_HMAC_SHA1_80"
INVALID = N.STATUS_DROP_INVALID


def rec(mask=0, ssrc=0, ts=0, seq=0, pt=0, reserved=0):
    return (mask, ssrc, ts, seq, pt, reserved)


def distinct(j, mask):
    """A record whose value bytes are all distinct and change with j."""
    return rec(mask, (0x11223344 + j * 0x00010001) & 0xFFFFFFFF, 0x55667788 ^ (j << 8 & 0xFFFF00), (0x99AA + j) & 0xFFFF,
               (0x3B + j) & 0xFF, 0xCC)


def setters(b, r):
    """RawPacket.setPayloadType / setSequenceNumber / setTimestamp / setSSRC on the bytes b (a numpy view)."""
    mask, ssrc, ts, seq, pt = (int(x) for x in tuple(r)[:5])
    if mask & PT:
        b[1] = (b[1] & 0x80) | (pt & 0x7F)
    if mask & SEQ:
        b[2:4] = list(seq.to_bytes(2, "big"))
    if mask & TS:
        b[4:8] = list(ts.to_bytes(4, "big"))
    if mask & SSRC:
        b[8:12] = list(ssrc.to_bytes(4, "big"))


class RwFan(Fan):
    """Fan with one record per entry: expand() applies the setters to each
    host-made copy of c >= 12 bytes; the engine's side passes the records."""

    def __init__(self, pkts, entries, records, **kw):
        super().__init__(pkts, entries, **kw)
        assert len(records) == self.n
        self.rw = np.array([tuple(r) for r in records], N.FANOUT_REWRITE_DTYPE).reshape(self.n)
        self.pass_records = True

    @classmethod
    def of(cls, fan, records):
        return cls(fan.pkts, list(zip(fan.src_idx.tolist(), fan.peers)), records)

    def copied(self, j):
        """c of entry j, or -1 when it is skipped."""
        if self.skipped(j)[0]:
            return -1
        si = int(self.src_idx[j])
        return min(int(self.src_len[si]), int(self.src_cap[si]), int(self.cap[j]))

    def applies(self, j):
        return self.copied(j) >= 12 and bool(int(self.rw["mask"][j]) & 0xF)

    def expand(self, rounded=False):
        seg, ln, fl = super().expand(rounded)
        for j in range(self.n):
            if self.applies(j):
                o = int(self.off[j])
                setters(seg[o:o + 12], self.rw[j])
        return seg, ln, fl

    def records(self):
        return self.rw if self.pass_records else None

    def run_host(self, eng):
        seg = np.full(self.seg_bytes, FILL, np.uint8)
        ln, st = eng.fanout_host_rw(self.tids, self.src_seg, self.src_off, self.src_len, self.src_cap, self.src_idx,
                                    seg, self.off, self.cap, self.src_status,
                                    self.flags if self.flags.any() else None, self.records())
        return seg, ln, st

    def run_device(self, eng, stream=None, misalign=0):
        import torch
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        src_seg = d(self.src_seg)
        seg = torch.full((self.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        args = [d(self.src_off), d(self.src_len), d(self.src_cap), d(self.src_idx), seg, d(self.off), ln, d(self.cap), st]
        rw = None
        if self.records() is not None:
            raw = torch.zeros(16 * self.n + 16, dtype=torch.uint8, device="cuda")
            rw = raw[misalign:misalign + 16 * self.n]
            rw.copy_(torch.from_numpy(self.rw.view(np.uint8).copy()))
        src_status = None if self.src_status is None else d(self.src_status)
        flags = d(self.flags) if self.flags.any() else None
        torch.cuda.synchronize()
        try:
            eng.fanout_device_rw(d(self.tids), src_seg, *args, rw, src_status=src_status, flags=flags, stream=stream)
        finally:
            eng.sync(stream)
            torch.cuda.synchronize()
            self.src_after = src_seg.cpu().numpy()
            self.seg_after = seg.cpu().numpy()
        return self.seg_after, ln.cpu().numpy().view(np.uint32), st.cpu().numpy()

    def ssrcs(self, j):
        """The SSRCs entry j bears on: its source's and, where the rewrite applies, the copy's."""
        si = int(self.src_idx[j])
        if not 0 <= si < self.m or len(self.pkts[si]) < 12:
            return []
        at = 8 if self.peers[j].kind == RTP else 4
        out = [int.from_bytes(self.pkts[si][at:at + 4], "big")]
        if self.applies(j) and int(self.rw["mask"][j]) & SSRC:
            out.append(int(self.rw["ssrc"][j]))
        return out

    def check(self, eng, got, ref=None, which=0):
        seg_r, ln_r, st_r = ref or self.reference()
        seg_e, ln_e, st_e = got
        assert st_e.tolist() == st_r.tolist(), [(j, int(a), int(b)) for j, (a, b) in enumerate(zip(st_e, st_r)) if a != b][:8]
        assert ln_e.tolist() == ln_r.tolist(), [(j, int(a), int(b)) for j, (a, b) in enumerate(zip(ln_e, ln_r)) if a != b][:8]
        for j in np.nonzero(st_r == 0)[0]:
            o, L = int(self.off[j]), int(ln_r[j])
            assert np.array_equal(seg_e[o:o + L], seg_r[o:o + L]), (int(j), int(self.src_idx[j]), L, self.rw[j])
        seen = set()
        for j, p in enumerate(self.peers):
            for ssrc in self.ssrcs(j):
                if (id(p), ssrc) in seen:
                    continue
                seen.add((id(p), ssrc))
                sr, se = p.r.state(ssrc), eng.context_state(p.e[which], ssrc)
                assert (sr is None) == (se is None), (j, hex(ssrc), sr, se)
                if sr is not None:
                    for k in (KEYS_RTP if p.kind == RTP else KEYS_RTCP):
                        assert int(se[k]) == int(sr[k]), (j, hex(ssrc), k, sr, se)
        return seg_r, ln_r, st_r


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


def region(f, seg, j):
    o = int(f.off[j])
    return seg[o:o + up16(f.cap[j])]


# ------------------------------------------------------------ 1. masks and lengths
LENGTHS = (12, 15, 16, 17, 28, 63, 64, 65, 1200)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("count", [27, 26, 1], ids=["n27", "n26", "n1"])
def test_masks_and_lengths(eng, route, count):
    """Every source length around the 16-byte piece that holds the header, and
    1200, to 3 peers; all 16 masks spread over the entries (5 j + 3 mod 16), the
    values of every record with distinct bytes; an odd and an even number of
    entries and a single one (a 12-byte source with every field set)."""
    peers = [Peer([eng], RTP, CM, seed()) for _ in range(3)]
    pk = [rtp(0x1000 + i, 7 + i, L) for i, L in enumerate(LENGTHS)]
    entries = ([(i, p) for i in range(len(pk)) for p in peers][:count]) if count > 1 else [(0, peers[1])]
    records = [distinct(j, (5 * j + 3) % 16 if count > 1 else 0xF) for j in range(len(entries))]
    assert count == 1 or {r[0] for r in records} == set(range(16))
    f = RwFan(pk, entries, records, room=16)
    got = f.run_host(eng) if route == "host" else f.run_device(eng)
    _, ln, st = f.check(eng, got)
    assert st.tolist() == [0] * f.n and ln.tolist() == [len(pk[e[0]]) + 10 for e in entries]
    if route == "device":
        assert np.array_equal(f.src_after, f.src_seg)


# ------------------------------------------------ 2. pair isolation and guard bytes
def test_pair_isolation_and_guard_bytes(engine_factory, oracle):
    """Wave pairs (entries 2k, 2k + 1) in a destination filled with a pattern,
    regions 16 and 48 bytes apart: a rewritten entry beside one the caller
    skipped, one skipped for its source's status, one with mask 0, and ones
    whose region holds 0, 8 and 11 bytes -- in both orders; the partners carry
    records with every field set, which must reach nothing.  A second identical
    engine gets the same fan-out through fanout_device, without records."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    a, b = (Peer([e1, e2], RTP, CM, seed()) for _ in range(2))
    pk = [rtp(0x2000 + i, 3 + i, L) for i, L in enumerate((28, 100, 17, 1200, 64, 40))]
    status = [0, 0, 0, 0, 0, N.STATUS_DROP_AUTH]
    R, Z, K = "rewritten", "mask 0", SKIP
    pairs = [((0, a, None, 0, R), (0, b, None, K, R)), ((5, a, None, 0, R), (1, b, None, 0, R)),
             ((2, a, None, 0, R), (2, b, None, 0, Z)), ((3, a, None, 0, R), (3, b, 0, 0, R)),
             ((1, a, None, 0, R), (4, b, 8, 0, R)), ((4, a, None, 0, R), (0, a, 11, 0, R)),
             # the same partners in front
             ((1, b, None, K, R), (3, b, None, 0, R)), ((2, b, 0, 0, R), (5, b, None, 0, R)),
             ((4, a, 11, 0, R), (5, a, None, 0, Z)), ((0, b, 8, 0, R), (2, a, 0, 0, R))]
    entries = [e[:4] for pr in pairs for e in pr]
    records = [distinct(j, 0xF if e[4] == R else 0) for j, e in enumerate(e for pr in pairs for e in pr)]
    f = RwFan(pk, entries, records, gaps=(16, 48), src_status=status, room=10)
    seg, ln, st = f.run_device(e1)
    f.check(e1, (seg, ln, st))
    plain = Fan(pk, entries, gaps=(16, 48), src_status=status, room=10)
    seg0, ln0, st0 = plain.run_device(e2)
    inside = np.zeros(f.seg_bytes, bool)
    short = 0
    for j in range(f.n):
        o, c = int(f.off[j]), up16(f.cap[j])
        si = int(f.src_idx[j])
        if f.skipped(j)[0]:
            assert st[j] == N.STATUS_SKIPPED and (seg[o:o + c] == FILL).all(), j
            continue
        inside[o:o + c] = True
        if f.cap[j] < 12:  # too short to patch: what fanout_device writes, byte for byte
            assert st[j] == INVALID and st0[j] == INVALID and ln[j] == ln0[j] == len(pk[si]), j
            assert np.array_equal(seg[o:o + c], seg0[o:o + c]), j
            assert np.array_equal(seg[o:o + c], f.src_seg[int(f.src_off[si]):][:c]), j
            short += 1
        elif not records[j][0]:  # mask 0: the source's header
            assert st[j] == 0 and np.array_equal(seg[o:o + 12], np.frombuffer(pk[si][:12], np.uint8)), j
        else:
            want = np.frombuffer(pk[si][:12], np.uint8).copy()
            setters(want, records[j])
            assert st[j] == 0 and np.array_equal(seg[o:o + 12], want), j
    assert (seg[~inside] == FILL).all() and (seg0[~inside] == FILL).all()
    assert short == 7 and sum(f.skipped(j)[0] for j in range(f.n)) == 5
    assert np.array_equal(f.src_after, f.src_seg)


# --------------------------------------------------------------- 3. too short to patch
def test_too_short_to_patch(engine_factory, oracle):
    """Sources of 8 and 11 bytes with every field set: DROP_INVALID and the
    bytes of the call without records."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    a = Peer([e1, e2], RTP, CM, seed())
    pk = [bytes([0x80, 96, 0, 1, 0, 0, 0, 0]), bytes([0x80, 96, 0, 2, 0, 0, 0, 9, 0xAA, 0xBB, 0xCC]), rtp(0x3000, 5, 28)]
    entries = [(0, a, 40), (1, a, 40), (2, a, 40), (1, a, 40), (0, a, 40)]
    f = RwFan(pk, entries, [distinct(j, 0xF) for j in range(5)], gaps=(16,))
    want = [INVALID, INVALID, 0, INVALID, INVALID]
    for route in ("device", "host"):
        got = f.run_device(e1) if route == "device" else f.run_host(e1)
        f.check(e1, got)
        assert got[2].tolist() == want and got[1].tolist() == [8, 11, 38, 11, 8]
        f.rw["seq"][2] += 1  # the next call's only valid packet is no replay
    seg0, ln0, st0 = Fan(pk, entries, gaps=(16,)).run_device(e2)
    assert st0.tolist() == want
    for j in (0, 1, 3, 4):
        assert np.array_equal(region(f, f.seg_after, j), region(f, seg0, j)), j
    assert e1.context_state(a.e[0], int(f.rw["ssrc"][0])) is None


# ------------------------------------------------------------ 4. the switch, with a wrap
@pytest.mark.parametrize("route", ["host", "device"])
def test_switch_with_wrap(eng, route):
    """A simulcast switch: SSRC A (seq 100..) then SSRC B (seq 5000..) are sent
    on as one stream T whose sequence numbers run 65533, 65534, 65535, 0, 1, 2
    across the switch, to an AES-CM and an AES-GCM peer.  T's context follows
    the rewritten numbers (ROC 1), and neither peer ever saw A or B."""
    A, B, T = 0x4A4A0001, 0x4B4B0002, 0x54545403
    peers = [Peer([eng], RTP, CM, seed()), Peer([eng], RTP, "AEAD_AES_128_GCM", seed())]
    pk = [rtp(A, 100 + i, 40 + i) for i in range(3)] + [rtp(B, 5000 + i, 50 + i) for i in range(3)]
    entries = [(i, p) for i in range(6) for p in peers]
    records = [rec(SSRC | SEQ | TS, T, 0x0BADF00D + 3000 * i, (65533 + i) & 0xFFFF) for i in range(6) for _ in peers]
    f = RwFan(pk, entries, records)
    got = f.run_host(eng) if route == "host" else f.run_device(eng)
    _, _, st = f.check(eng, got)
    assert st.tolist() == [0] * 12
    for p in peers:
        sr, se = p.r.state(T), eng.context_state(p.e[0], T)
        assert int(sr["roc"]) == 1 and int(se["roc"]) == 1 and int(se["s_l"]) == 2
        for ssrc in (A, B):
            assert p.r.state(ssrc) is None and eng.context_state(p.e[0], ssrc) is None


# ------------------------------------------------------------------- 5. replay by target
def test_replay_by_target(eng):
    """The same source twice toward one transformer: under two rewritten
    sequence numbers both are sent; under the same record the second is a
    replay (the reference's sender checks replays too)."""
    a, b = (Peer([eng], RTP, CM, seed()) for _ in range(2))
    pk = [rtp(0x5000, 10, 60), rtp(0x5001, 11, 60)]
    entries = [(0, a), (0, a), (1, b), (1, b), (1, a), (1, a)]
    same = rec(SSRC | SEQ, 0x5B5B0001, 0, 700)
    records = [rec(SEQ, 0, 0, 20), rec(SEQ, 0, 0, 21), same, same, rec(0), rec(PT, pt=100)]
    f = RwFan(pk, entries, records)
    _, _, st = f.check(eng, f.run_host(eng))
    assert st.tolist() == [0, 0, 0, N.STATUS_DROP_REPLAY, 0, N.STATUS_DROP_REPLAY]


# ---------------------------------------------------------------------- 6. every profile
def profile_records(f):
    """RTP entries rewritten, SRTCP entries mask 0.  A context keeps one mask
    (chosen by peer and source SSRC), so its sequence numbers stay in order: the
    target SSRC maps the 16 source SSRCs one to one, the target sequence number
    is the source's + 1000."""
    order = {}
    records = []
    for j, p in enumerate(f.peers):
        pkt = f.pkts[int(f.src_idx[j])]
        if p.kind == RTCP:
            records.append(rec(0, 0xDEAD0000 + j, j, j & 0xFFFF, j & 0xFF))
            continue
        k = order.setdefault(id(p), len(order))
        ssrc, seq = int.from_bytes(pkt[8:12], "big"), int.from_bytes(pkt[2:4], "big")
        mask = (5 * (16 * k + (ssrc & 15)) + 3) % 16
        records.append(rec(mask, 0x7000 + (ssrc & 15), 0x01020304 * (j % 60 + 1), seq + 1000, (j * 3) & 0xFF, j & 0xFF))
    return records


def test_every_profile(engine_factory, oracle):
    """profile_fan's mix at n = 200: senders of every SRTP profile with their
    RTP entries rewritten, and SRTCP entries with mask 0 in the same bundle.
    Held to the references and, bit for bit over the whole destination segment,
    to a twin engine that gets the host-made copies through transform_device."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    f0 = profile_fan([e1, e2], 200, RTP_PROFILES, RTCP_PROFILES)
    f = RwFan.of(f0, profile_records(f0))
    assert {int(m) for m, p in zip(f.rw["mask"], f.peers) if p.kind == RTP} == set(range(16))
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert st.tolist() == [0] * 200
    twin_equal(f, e2, got)


# ---------------------------------------------------------------------- 7. the stride loop
def test_stride_loop(engine_factory, oracle):
    """n = 32768 + 5: only above 32768 entries (4096 workgroups of four waves,
    two entries a wave) does a wave take a second pair, and the record index
    has to move with it.  28-byte sources, a record of its own for every entry."""
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, CM, seed())
    n = 32768 + 5
    pk = [rtp(0x6000 + i, 9, 28) for i in range(64)]
    entries = [(j % 64, a, 48) for j in range(n)]
    records = [rec(0xF, 0x00700000 + (j % 4096), (j * 2654435761) & 0xFFFFFFFF, 1 + j // 4096, j % 128) for j in range(n)]
    f = RwFan(pk, entries, records)
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert not st.any()
    # every copy's header carries its own record: the last five entries too
    hdr = got[0].reshape(n, 48)[:, :12]
    assert (hdr[:, 1] == (np.arange(n) % 128)).all()
    assert (hdr[:, 2].astype(int) * 256 + hdr[:, 3] == 1 + np.arange(n) // 4096).all()
    assert (hdr[:, 8:12].copy().view(">u4")[:, 0] == 0x00700000 + np.arange(n) % 4096).all()
    assert (hdr[:, 4:8].copy().view(">u4")[:, 0] == (np.arange(n, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF).all()


# ---------------------------------------------------- 8. on the device after a receive
def test_forward_on_device_rewritten(eng):
    """test_forward_on_device's shape with records: transform_device(reverse)
    on the engine's stream, then fanout_device_rw on the same stream with that
    call's length and status tensors as src_len and src_status and no
    synchronise between the two; every peer gets the packets under its own
    target SSRCs and payload type, with a replaced timestamp."""
    import torch
    snd = Peer([eng], RTP, CM, seed())
    rcv = Peer([eng], RTP, CM, TF._seed[0], sender=False)  # the same keys
    peers = [Peer([eng], RTP, CM, seed()), Peer([eng], RTP, "AEAD_AES_128_GCM", seed()),
             Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_32", seed())]
    clear = [rtp(0x5000 + (i % 4), 100 + i // 4, 40 + 9 * (i % 7)) for i in range(64)]
    seg, off, ln, cap = G.pack(clear, room=16)
    assert O.process(snd.r, False, seg, off, ln, cap).tolist() == [0] * 64
    wire = [seg[off[i]:off[i] + ln[i]].tobytes() for i in range(64)]
    for i in (9, 40):  # forged
        b = bytearray(wire[i])
        b[-1 if i == 9 else 20] ^= 4
        wire[i] = bytes(b)
    wire[17], wire[50] = wire[5], wire[30]  # replayed
    wire[33] = bytes([0x40]) + wire[33][1:]  # version 1
    w_seg, w_off, w_len, w_cap = G.pack(wire, room=0)
    u_seg, u_len = w_seg.copy(), w_len.copy()
    u_st = O.process(rcv.r, True, u_seg, w_off, u_len, w_cap)
    assert sorted(np.nonzero(u_st)[0].tolist()) == [9, 17, 33, 40, 50]
    entries = [(i, p) for i in range(64) for p in peers]
    records = [rec(SSRC | TS | PT, 0x51000000 + 0x100 * k + (i % 4), 0xCAFE0000 + 7 * i, 0, 100 + k)
               for i in range(64) for k in range(3)]
    f = RwFan(wire, entries, records, src_len=u_len, src_status=u_st)
    f.src_seg = u_seg  # the sources as the unprotect left them
    ref = f.reference()
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    s = eng.stream_ptr
    r_seg, r_len, r_st = d(w_seg), d(w_len), torch.full((64,), -1, dtype=torch.int32, device="cuda")
    r_off, r_cap = d(w_off), d(w_cap)
    o_seg = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
    o_len = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_st = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_idx, o_tids, o_off, o_cap = d(f.src_idx), d(f.tids), d(f.off), d(f.cap)
    o_rw = torch.from_numpy(f.rw.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    eng.transform_device(True, rcv.tid, r_seg, r_off, r_len, r_cap, r_st, stream=s)
    eng.fanout_device_rw(o_tids, r_seg, r_off, r_len, r_cap, o_idx, o_seg, o_off, o_len, o_cap, o_st, o_rw,
                         src_status=r_st, stream=s)
    eng.sync(s)
    torch.cuda.synchronize()
    assert r_st.cpu().numpy().tolist() == u_st.tolist()
    assert np.array_equal(r_seg.cpu().numpy(), u_seg)  # the received bundle is not written by the fan-out
    f.check(eng, (o_seg.cpu().numpy(), o_len.cpu().numpy().view(np.uint32), o_st.cpu().numpy()), ref)
    assert (ref[2].reshape(64, 3) == np.where(u_st != 0, 9, 0)[:, None]).all()
    for k, p in enumerate(peers):
        assert eng.context_state(p.e[0], 0x5000) is None
        assert eng.context_state(p.e[0], 0x51000000 + 0x100 * k) is not None


# ------------------------------------------------- 9. nothing changes without records
def test_nothing_changes_without_records(engine_factory, oracle):
    """fanout_device_rw with rewrite=None, and with records whose masks are all
    0 (and whose values are not), against fanout_device on identical engines:
    statuses, lengths and the whole destination segment bit for bit, and all of
    them equal to the rounded host-made copies through transform_device."""
    engs = [make_engine(engine_factory) for _ in range(4)]
    f0 = profile_fan(engs, 200, RTP_PROFILES, RTCP_PROFILES)
    got = f0.run_device(engs[0])
    f = RwFan.of(f0, [rec(0, 0x11223344, 0x55667788, 0x99AA, 0xBB, 0xCC)] * f0.n)
    f.pass_records = False
    none = f.run_device(engs[1])
    f.pass_records = True
    zero = f.run_device(engs[2])
    assert got[2].tolist() == [0] * 200
    for other in (none, zero):
        assert other[2].tolist() == got[2].tolist() and other[1].tolist() == got[1].tolist()
        assert np.array_equal(other[0], got[0])
    twin_equal(f, engs[3], zero)


# ------------------------------------------------------------------ 10. argument rules
def test_argument_rules(engine_factory, oracle):
    """A device array misaligned by 4 bytes and a mask of 0x10 on the host
    route are SRTP_EINVAL with nothing changed; on the device route, where the
    records are not read back, a mask of 0x1F behaves as 0xF."""
    e1 = make_engine(engine_factory)
    a = Peer([e1], RTP, CM, seed())
    pk = [rtp(0x8000 + i, 4, 44) for i in range(3)]
    entries = [(i, a) for i in range(3)]
    f = RwFan(pk, entries, [distinct(j, 0x1F) for j in range(3)])
    st0 = e1.fanout_stats()
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        f.run_device(e1, misalign=4)
    assert (f.seg_after == FILL).all() and np.array_equal(f.src_after, f.src_seg)
    g = RwFan(pk, entries, [distinct(0, 0xF), distinct(1, 0x10), distinct(2, 0xF)])
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        g.run_host(e1)
    assert e1.fanout_stats() == st0
    for r in (f, g):
        for j in range(3):
            for ssrc in r.ssrcs(j) + [int(r.rw["ssrc"][j])]:
                assert e1.context_state(a.e[0], ssrc) is None
    seg, ln, st = f.run_device(e1)  # aligned: bits above 0xF are ignored
    f.check(e1, (seg, ln, st))
    assert st.tolist() == [0, 0, 0]
    for j in range(3):
        want = np.frombuffer(pk[j][:12], np.uint8).copy()
        setters(want, distinct(j, 0xF))
        assert np.array_equal(seg[int(f.off[j]):][:12], want)
    assert e1.fanout_stats()["calls"] == st0["calls"] + 1


# ------------------------------------------------------------------------ 11. fan_out_rw()
class Switcher:
    """A stateful rewriter in SsrcRewriter's manner: every source SSRC is sent
    on as one target SSRC with sequence numbers that continue across sources."""

    def __init__(self, target, first_seq):
        self.target, self.next = target, first_seq

    def __call__(self, pkt):
        seq = self.next & 0xFFFF
        self.next += 1
        return {"ssrc": self.target, "seq": seq, "timestamp": 0x1000 * seq}


class DropOdd:
    """rewriteRTP returning null for packets with an odd sequence number; the others keep all but the payload type."""

    def __call__(self, pkt):
        d = pkt.data()
        return None if d[3] & 1 else {"pt": 111}


def rewritten_copy(raw, r):
    b = np.frombuffer(raw, np.uint8).copy()
    setters(b, rec(sum(bit for name, bit in (("ssrc", SSRC), ("seq", SEQ), ("timestamp", TS), ("pt", PT)) if name in r),
                   r.get("ssrc", 0), r.get("timestamp", 0), r.get("seq", 0), r.get("pt", 0)))
    return RawPacket(b.tobytes(), 0, len(raw))


def test_fan_out_rw_api(engine_factory, oracle):
    """fan_out_rw against each transformer's own transform() of host-made,
    host-rewritten copies on a twin engine.  One rewriter is shared by two
    transformers and stateful (its numbers show doWrite's order: packet by
    packet, stream by stream), one returns None for some packets and an empty
    mapping's equal for none, one transformer has no rewriter."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    peers = [Peer([e1, e2], RTP, name, seed()) for name in (CM, "AEAD_AES_256_GCM", CM, "F8_128_HMAC_SHA1_80")]
    raw = [rtp(0x6000 + (i & 1), 30 + i, 50 + 13 * i) for i in range(5)]
    pkts = [RawPacket(b"\x00" * 3 + r, 3, len(r)) if i != 2 else None for i, r in enumerate(raw)]
    before = [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts]
    shared = Switcher(0x7A7A0001, 65530)
    out = fan_out_rw(pkts, [p.e[0] for p in peers], [shared, shared, DropOdd(), None])
    assert [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts] == before
    assert len(out) == 4 and shared.next == 65530 + 8
    # the host's way: the rewriters run in doWrite's order over host-made copies
    model, drop = Switcher(0x7A7A0001, 65530), DropOdd()
    copies = [[None] * 5 for _ in peers]
    for i, p in enumerate(pkts):
        if p is None:
            continue
        for k, f in enumerate((model, model, drop, lambda pkt: {})):
            r = f(p)
            copies[k][i] = None if r is None else rewritten_copy(raw[i], r)
    assert [c is None for c in copies[2]] == [False, True, True, True, False]
    for k, p in enumerate(peers):
        want = p.e[1].transform(copies[k])
        for i in range(5):
            assert (out[k][i] is None) == (want[i] is None), (k, i)
            if want[i] is not None:
                assert out[k][i].data() == want[i].data(), (k, i)
    for k in (0, 1):  # the shared stream wrapped on both peers; neither saw the source SSRCs
        got, ref = e1.context_state(peers[k].e[0], 0x7A7A0001), e2.context_state(peers[k].e[1], 0x7A7A0001)
        for key in KEYS_RTP:
            assert got[key] == ref[key]
        assert got["roc"] == 1 and e1.context_state(peers[k].e[0], 0x6000) is None
    with pytest.raises(ValueError):
        fan_out_rw(pkts, [p.e[0] for p in peers], [None, None, None, lambda pkt: {"marker": 1}])
