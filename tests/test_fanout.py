"""Fan-out on the device (srtp_fanout_device / _host, k_fanout, fan_out()): m
source packets, n destination entries of (source index, transformer,
destination region), protected as if each were a host-made copy of its source.

The expected result is always built the obvious way: the entries are expanded
on the host with numpy (len = src_len[src_idx], the bytes copied, SKIP where
the rule says) and that bundle goes through the reference -- oracle.process for
the RFC 3711 / ZRTP profiles, gcm_ref.process for AES-GCM (contexts belong to
transformers, so the two references each take their transformers' entries, in
order).  Compared: status and length of every entry, the bytes [off, off + len)
of every OK entry, and the state of every (transformer, SSRC) context."""
import numpy as np
import pytest

import gcm_ref as G
from libjitsi_amd import (RawPacket, SRTCPTransformer, SRTPContextFactory, SRTPPolicy, SRTPTransformer, fan_out,
                          profile_policies)
from libjitsi_amd import _native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTP, RTCP = 0, 1
KEYS_RTP = ("roc", "s_l", "seq_num_set", "guessed_roc", "replay_window")
KEYS_RTCP = ("sent_index", "received_index", "replay_window")
FILL = 0xA5
SKIP = N.PKT_FLAG_SKIP
GCM = {"AEAD_AES_128_GCM": 16, "AEAD_AES_256_GCM": 32}


def tup(p: SRTPPolicy):
    return (p.encType, p.encKeyLength, p.authType, p.authKeyLength, p.authTagLength, p.saltKeyLength)


class Peer:
    """One transformer (a peer's sender) in the reference and in each engine of `engs`."""

    def __init__(self, engs, kind, profile, seed, sender=True):
        sp, cp = (tup(p) for p in profile_policies(profile))
        self.kind, self.gcm = kind, profile in GCM
        mk = G.payload(32 if sp[1] == 32 else 16, 7000 + seed)
        ms = G.payload(12 if self.gcm else 14, 8000 + seed)
        if self.gcm:
            self.r = G.Transformer(kind, *[G.Factory(sender, mk, ms, sp, cp)] * 2)
        else:
            f = O.Factory(sender, mk, ms, O.Policy(*sp), O.Policy(*cp))
            self.r = O.Transformer(kind, f, f)
        cls = SRTPTransformer if kind == RTP else SRTCPTransformer
        self.e = []
        for eng in engs:
            f = SRTPContextFactory(sender, mk, ms, SRTPPolicy(*sp), SRTPPolicy(*cp), engine=eng)
            self.e.append(cls(f, f))
        self.tid = self.e[0].tid
        assert all(t.tid == self.tid for t in self.e)  # twin engines are built alike


def up16(v):
    return (int(v) + 15) & ~15


def layout(caps, gaps=(0,)):
    """Region offsets for the capacities, `gaps[j % len]` bytes between regions."""
    off, pos = np.zeros(len(caps), np.uint32), 0
    for j, c in enumerate(caps):
        off[j] = pos
        pos += up16(c) + gaps[j % len(gaps)]
    return off, max(pos, 16)


class Fan:
    """A fan-out's arrays: sources packed without room (a received bundle) and
    destination entries (src_idx, peer, cap, flags)."""

    def __init__(self, pkts, entries, gaps=(0,), src_len=None, src_status=None, room=None):
        self.pkts = pkts
        self.src_seg, self.src_off, self.src_len, self.src_cap = G.pack(pkts, room=0)
        if src_len is not None:
            self.src_len = np.asarray(src_len, np.uint32)
        self.src_status = None if src_status is None else np.asarray(src_status, np.int32)
        self.m, self.n = len(pkts), len(entries)
        self.src_idx = np.array([e[0] for e in entries], np.int32)
        self.peers = [e[1] for e in entries]
        self.tids = np.array([p.tid for p in self.peers], np.int32)

        def cap_of(e):
            if len(e) > 2 and e[2] is not None:
                return e[2]
            L = int(self.src_len[e[0]]) if 0 <= e[0] < self.m else 32
            return min(L + 24 if room is None else L + room, 65535)
        self.cap = np.array([cap_of(e) for e in entries], np.uint32)
        self.flags = np.array([e[3] if len(e) > 3 else 0 for e in entries], np.uint32)
        self.off, self.seg_bytes = layout(self.cap, gaps)

    def skipped(self, j):
        si = int(self.src_idx[j])
        by_source = not 0 <= si < self.m or (self.src_status is not None and self.src_status[si] != 0)
        return by_source or bool(self.flags[j] & SKIP), by_source

    def expand(self, rounded=False):
        """The host-made copies: (seg, len, flags).  rounded: the copy rounded
        up to 16 bytes as k_fanout moves it (for whole-segment comparisons)."""
        seg = np.full(self.seg_bytes, FILL, np.uint8)
        ln, fl = np.zeros(self.n, np.uint32), self.flags.copy()
        for j in range(self.n):
            if self.skipped(j)[0]:
                fl[j] |= SKIP
                continue
            si = int(self.src_idx[j])
            ln[j] = self.src_len[si]
            c = min(int(ln[j]), int(self.src_cap[si]), int(self.cap[j]))
            c = up16(c) if rounded else c
            so, do = int(self.src_off[si]), int(self.off[j])
            seg[do:do + c] = self.src_seg[so:so + c]
        return seg, ln, fl

    def reference(self):
        """(seg, len, status) of the expanded bundle under the references."""
        seg, ln, fl = self.expand()
        st = np.zeros(self.n, np.int32)
        for gcm, proc in ((False, O.process), (True, G.process)):
            idx = [j for j in range(self.n) if self.peers[j].gcm == gcm]
            if not idx:
                continue
            sub_ln = np.ascontiguousarray(ln[idx])
            st[idx] = proc([self.peers[j].r for j in idx], False, seg, np.ascontiguousarray(self.off[idx]), sub_ln,
                           np.ascontiguousarray(self.cap[idx]), np.ascontiguousarray(fl[idx]), True)
            ln[idx] = sub_ln
        return seg, ln, st

    # ---- the engine's side
    def run_host(self, eng):
        seg = np.full(self.seg_bytes, FILL, np.uint8)
        ln, st = eng.fanout_host(self.tids, self.src_seg, self.src_off, self.src_len, self.src_cap, self.src_idx, seg,
                                 self.off, self.cap, self.src_status, self.flags if self.flags.any() else None)
        return seg, ln, st

    def run_device(self, eng, stream=None):
        import torch
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        src_seg = d(self.src_seg)
        seg = torch.full((self.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
        ln = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        args = [d(self.src_off), d(self.src_len), d(self.src_cap), d(self.src_idx), seg, d(self.off), ln, d(self.cap), st]
        tids = d(self.tids)
        src_status = None if self.src_status is None else d(self.src_status)
        flags = d(self.flags) if self.flags.any() else None
        torch.cuda.synchronize()
        eng.fanout_device(tids, src_seg, *args, src_status=src_status, flags=flags, stream=stream)
        eng.sync(stream)
        torch.cuda.synchronize()
        self.src_after = src_seg.cpu().numpy()
        return seg.cpu().numpy(), ln.cpu().numpy().view(np.uint32), st.cpu().numpy()

    def check(self, eng, got, ref=None, which=0):
        seg_r, ln_r, st_r = ref or self.reference()
        seg_e, ln_e, st_e = got
        assert st_e.tolist() == st_r.tolist(), [(j, int(a), int(b)) for j, (a, b) in enumerate(zip(st_e, st_r)) if a != b][:8]
        assert ln_e.tolist() == ln_r.tolist(), [(j, int(a), int(b)) for j, (a, b) in enumerate(zip(ln_e, ln_r)) if a != b][:8]
        for j in np.nonzero(st_r == 0)[0]:
            o, L = int(self.off[j]), int(ln_r[j])
            assert np.array_equal(seg_e[o:o + L], seg_r[o:o + L]), (int(j), int(self.src_idx[j]), L)
        seen = set()
        for j, p in enumerate(self.peers):
            si = int(self.src_idx[j])
            if not 0 <= si < self.m or len(self.pkts[si]) < 12:
                continue
            at = 8 if p.kind == RTP else 4
            ssrc = int.from_bytes(self.pkts[si][at:at + 4], "big")
            if (id(p), ssrc) in seen:
                continue
            seen.add((id(p), ssrc))
            sr, se = p.r.state(ssrc), eng.context_state(p.e[which], ssrc)
            assert (sr is None) == (se is None), (j, hex(ssrc), sr, se)
            if sr is not None:
                for k in (KEYS_RTP if p.kind == RTP else KEYS_RTCP):
                    assert int(se[k]) == int(sr[k]), (j, hex(ssrc), k, sr, se)
        return seg_r, ln_r, st_r


def make_engine(engine_factory, **kw):
    e = engine_factory(max_contexts=1 << 15, max_factories=256, max_transformers=1024, **kw)
    e.enable_aead()
    O.set_check_replay(True)
    return e


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


_seed = [0]


def seed():
    _seed[0] += 1
    return _seed[0]


def rtp(ssrc, seq, n):
    """An RTP packet of n bytes in all."""
    return G.rtp_packet(ssrc, seq, G.payload(n - 12, ssrc + seq))


# ------------------------------------------------------- 1. lengths and strides
LENGTHS = (12, 15, 16, 17, 28, 63, 64, 65, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 4097, 65519)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("sources", [17, 16, 1], ids=["n51", "n48", "n1"])
def test_lengths_and_strides(eng, route, sources):
    """Every source length around the 16-byte, the 1 KB (a wave-instruction) and
    the 2 KB (a trip) strides and the largest a region can hold, each on its own
    SSRC, to N = 3 peers of one AES_CM_128_HMAC_SHA1_80 sender profile; an odd
    and an even number of entries (the pair tail) and a single one."""
    peers = [Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed()) for _ in range(3)]
    pk = [rtp(0x1000 + i, 7 + i, L) for i, L in enumerate(LENGTHS[:sources])]
    entries = [(i, p) for i in range(len(pk)) for p in peers] if sources > 1 else [(0, peers[1])]
    f = Fan(pk, entries, room=16)
    got = f.run_host(eng) if route == "host" else f.run_device(eng)
    _, ln, st = f.check(eng, got)
    assert st.tolist() == [0] * f.n and ln.tolist() == [len(pk[e[0]]) + 10 for e in entries]


# ------------------------------------------------------------ 2. untouched bytes
def test_untouched_bytes_device(eng):
    """Regions 16 and 48 bytes apart in a destination filled with a pattern:
    after the call every byte outside all regions holds it, the regions of
    skipped entries hold it too, and the source tensor is unchanged."""
    peers = [Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed()) for _ in range(3)]
    pk = [rtp(0x2000 + i, 3 + i, L) for i, L in enumerate((12, 17, 100, 1025, 2049, 31))]
    status = [0, 0, 2, 0, 0, 0]
    entries = [(i, p, None, SKIP if (i, k) == (3, 1) else 0) for i in range(len(pk)) for k, p in enumerate(peers)]
    entries.insert(4, (len(pk), peers[0], 64))  # names no source
    f = Fan(pk, entries, gaps=(16, 48), src_status=status, room=10)  # cap = len + the 10-byte tag, not a multiple of 16
    seg, ln, st = f.run_device(eng)
    f.check(eng, (seg, ln, st))
    inside = np.zeros(f.seg_bytes, bool)
    for j in range(f.n):
        o, c = int(f.off[j]), up16(f.cap[j])
        if f.skipped(j)[0]:
            assert st[j] == N.STATUS_SKIPPED and (seg[o:o + c] == FILL).all(), j
        else:
            inside[o:o + c] = True
    assert (seg[~inside] == FILL).all()
    assert sum(f.skipped(j)[0] for j in range(f.n)) == 3 + 1 + 1
    assert np.array_equal(f.src_after, f.src_seg)


# --------------------------------------------------------- 3. gating and rejects
def test_gating_and_rejects(eng):
    """Non-OK sources, an out-of-range index (device: SKIPPED; host: EINVAL,
    nothing launched), a caller SKIP flag, a region smaller than the source
    (DROP_INVALID), one a byte short of the trailer (ERR_CAPACITY), an 8-byte
    source, the same source twice toward one transformer (the second a replay:
    the reference's sender checks replays too) and a source nobody gets."""
    a, b = (Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed()) for _ in range(2))
    pk = [rtp(0x3000, 10, 60), rtp(0x3000, 11, 60), rtp(0x3000, 12, 60), rtp(0x3001, 5, 100), rtp(0x3001, 6, 100),
          bytes([0x80, 96, 0, 1, 0, 0, 0, 0]), rtp(0x3002, 9, 40), rtp(0x3003, 1, 40), rtp(0x3004, 2, 40)]
    status = [0, N.STATUS_DROP_AUTH, N.STATUS_DROP_REPLAY, 0, 0, 0, 0, 0, 0]
    entries = [(0, a), (0, b), (1, a), (1, b), (2, a),
               (3, a, 99), (3, b, 100), (4, a, 109), (4, b, 110),  # cap < len; no trailer room; one short; enough
               (5, a), (6, a), (6, a), (6, b), (8, a, None, SKIP), (8, b)]  # source 7 goes to nobody
    f = Fan(pk, entries, src_status=status)
    ref = f.reference()
    want = [0, 0, 9, 9, 9, 7, 5, 5, 0, 7, 0, 1, 0, 9, 0]
    assert ref[2].tolist() == want
    st0 = eng.fanout_stats()
    f.check(eng, f.run_host(eng), ref)
    st1 = eng.fanout_stats()
    assert st1["calls"] == st0["calls"] + 1 and st1["sources"] == st0["sources"] + 9
    assert st1["destinations"] == st0["destinations"] + 15 and st1["skipped"] == st0["skipped"] + 3
    assert st1["src_bytes_h2d"] == st0["src_bytes_h2d"] + f.src_seg.nbytes
    # the device route, fresh peers (the first two now hold these packets' indices), with indices that name no source
    a2, b2 = (Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed()) for _ in range(2))
    swap = {id(a): a2, id(b): b2}
    entries2 = [(e[0], swap[id(e[1])]) + tuple(e[2:]) for e in entries]
    for k, bad in ((2, len(pk)), (7, -1), (15, 2 ** 31 - 1), (18, -2 ** 31)):
        entries2.insert(k, (bad, a2, 48))
    f2 = Fan(pk, entries2, src_status=status)
    ref2 = f2.reference()
    assert [s for j, s in enumerate(ref2[2].tolist()) if 0 <= f2.src_idx[j] < len(pk)] == want
    f2.check(eng, f2.run_device(eng), ref2)
    st2 = eng.fanout_stats()
    assert st2["skipped"] == st1["skipped"] + 3 + 4 and st2["src_bytes_h2d"] == st1["src_bytes_h2d"]
    # the host route refuses them before anything is launched
    with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
        f2.run_host(eng)
    f3 = Fan(pk[:1], [(0, a2)])
    for m_bad in (dict(src_off=np.array([8], np.uint32)), dict(src_cap=np.array([70000], np.uint32)),
                  dict(off=np.array([f3.seg_bytes], np.uint32))):
        for k, v in m_bad.items():
            setattr(f3, k, v)
        with pytest.raises(N.SrtpError, match="SRTP_EINVAL"):
            f3.run_host(eng)
        f3 = Fan(pk[:1], [(0, a2)])
    assert eng.fanout_stats() == st2
    assert eng.context_state(a2.e[0], 0x3003) is None  # the source nobody got


# ------------------------------------------------- 4. every profile, every route
RTP_PROFILES = ("AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM", "F8_128_HMAC_SHA1_80", "TWOFISH_CM_128_SKEIN_32",
                "AES_CM_128_HMAC_SHA1_32", "AES_256_CM_HMAC_SHA1_80", "NULL_HMAC_SHA1_80", "AEAD_AES_256_GCM")
RTCP_PROFILES = ("AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM")
CM_ONLY = ("AES_CM_128_HMAC_SHA1_80", "AES_CM_128_HMAC_SHA1_32", "NULL_HMAC_SHA1_80")


def profile_fan(engs, n, rtp_profiles, rtcp_profiles):
    """n entries, source-major: 200-byte RTP sources toward the SRTP peers and
    200-byte RTCP sources toward the SRTCP peers, each (source, peer) once.  In
    the large bundles an AES-GCM peer gets every seventh source only: gcm_ref
    hashes bit by bit in Python."""
    rp = [Peer(engs, RTP, name, seed()) for name in rtp_profiles]
    cp = [Peer(engs, RTCP, name, seed()) for name in rtcp_profiles]
    pk, entries, i = [], [], 0
    while len(entries) < n:
        if i % 6 == 5:
            pk.append(G.rtcp_packet(0x4800 + (i % 3), G.payload(192, i)))
            dst = cp
        else:
            pk.append(rtp(0x4000 + (i % 16), 20 + i // 16, 200))
            dst = rp
        entries += [(i, p) for p in dst if not (p.gcm and n > 200 and i % 7)]
        i += 1
    return Fan(pk, entries[:n])


@pytest.mark.parametrize("n", [4, 200, 2560])
def test_every_profile(engine_factory, oracle, n):
    """One fan-out's destinations over senders of _80, _32, AES-256-CM, F8, the
    NULL cipher, Twofish + Skein, GCM-128 and GCM-256 SRTP, and AES-CM and GCM
    SRTCP transformers with SRTCP sources: k_small's range, the chain, and a
    bundle past the wave-per-packet sizes' small end.  Held to the references
    and, bit for bit over the whole destination segment, to a second identical
    engine that gets the host-expanded bundle through transform_device."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    f = profile_fan([e1, e2], n, RTP_PROFILES, RTCP_PROFILES)
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert st.tolist() == [0] * n
    twin_equal(f, e2, got)


@pytest.mark.parametrize("n", [4, 200, 2560])
def test_cm_only_engine(engine_factory, oracle, n):
    """An engine that holds only AES-CM / NULL-cipher + HMAC-SHA1 key sets: the
    protect chain runs n = 4 and 200 in one launch (k_small) and n = 2560 on
    the split path (k_ctr_wide + k_mac_wide)."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    f = profile_fan([e1, e2], n, CM_ONLY, CM_ONLY[:1])
    got = f.run_device(e1)
    _, _, st = f.check(e1, got)
    assert st.tolist() == [0] * n
    twin_equal(f, e2, got)
    assert e1.stats()["small_bundles"] == (1 if n <= 255 else 0)


def twin_equal(f, e2, got):
    import torch
    seg_h, ln_h, fl_h = f.expand(rounded=True)
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    seg, ln, st = d(seg_h), d(ln_h), torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    e2.transform_device(False, d(f.tids), seg, d(f.off), ln, d(f.cap), st, flags=d(fl_h))
    e2.sync()
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == got[2].tolist()
    assert ln.cpu().numpy().view(np.uint32).tolist() == got[1].tolist()
    assert np.array_equal(seg.cpu().numpy(), got[0])


# ------------------------------------------------- 5. forwarding on the device
def test_forward_on_device(eng):
    """A received bundle is unprotected and forwarded with no host in between:
    transform_device(reverse) on the engine's stream, then fanout_device on the
    same stream with that call's length and status tensors as src_len and
    src_status, to 3 peers (one AES-GCM), source-major.  64 wire packets over 4
    SSRCs from a twin sender, two of them forged, two replayed, one with a bad
    version: their copies are skipped."""
    import torch
    snd = Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed())
    rcv = Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", _seed[0], sender=False)  # the same keys
    peers = [Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", seed()), Peer([eng], RTP, "AEAD_AES_128_GCM", seed()),
             Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_32", seed())]
    clear = [rtp(0x5000 + (i % 4), 100 + i // 4, 40 + 9 * (i % 7)) for i in range(64)]
    seg, off, ln, cap = G.pack(clear, room=16)
    assert O.process(snd.r, False, seg, off, ln, cap).tolist() == [0] * 64
    wire = [seg[off[i]:off[i] + ln[i]].tobytes() for i in range(64)]
    for i in (9, 40):  # forged: a bit of the tag, a bit of the payload
        b = bytearray(wire[i])
        b[-1 if i == 9 else 20] ^= 4
        wire[i] = bytes(b)
    wire[17], wire[50] = wire[5], wire[30]  # replayed (same SSRCs: 17 % 4 == 5 % 4, 50 % 4 == 30 % 4)
    wire[33] = bytes([0x40]) + wire[33][1:]  # version 1
    w_seg, w_off, w_len, w_cap = G.pack(wire, room=0)
    # the reference: unprotect, then protect of the accepted packets per peer
    u_seg, u_len = w_seg.copy(), w_len.copy()
    u_st = O.process(rcv.r, True, u_seg, w_off, u_len, w_cap)
    assert sorted(np.nonzero(u_st)[0].tolist()) == [9, 17, 33, 40, 50] and u_st[33] == N.STATUS_DROP_VERSION
    entries = [(i, p) for i in range(64) for p in peers]
    f = Fan(wire, entries, src_len=u_len, src_status=u_st)
    f.src_seg = u_seg  # the sources as the unprotect left them
    ref = f.reference()
    # the engine: both calls on its own stream, the tensors of the first feed the second
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    s = eng.stream_ptr
    st0 = eng.fanout_stats()
    r_seg, r_len, r_st = d(w_seg), d(w_len), torch.full((64,), -1, dtype=torch.int32, device="cuda")
    r_off, r_cap = d(w_off), d(w_cap)
    o_seg = torch.full((f.seg_bytes,), FILL, dtype=torch.uint8, device="cuda")
    o_len = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_st = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
    o_idx, o_tids, o_off, o_cap = d(f.src_idx), d(f.tids), d(f.off), d(f.cap)
    torch.cuda.synchronize()
    eng.transform_device(True, rcv.tid, r_seg, r_off, r_len, r_cap, r_st, stream=s)
    eng.fanout_device(o_tids, r_seg, r_off, r_len, r_cap, o_idx, o_seg, o_off, o_len, o_cap, o_st, src_status=r_st,
                      stream=s)
    eng.sync(s)
    torch.cuda.synchronize()
    assert r_st.cpu().numpy().tolist() == u_st.tolist()
    f.check(eng, (o_seg.cpu().numpy(), o_len.cpu().numpy().view(np.uint32), o_st.cpu().numpy()), ref)
    assert (ref[2].reshape(64, 3) == np.where(u_st != 0, 9, 0)[:, None]).all()
    st1 = eng.fanout_stats()
    assert st1["sources"] == st0["sources"] + 64 and st1["destinations"] == st0["destinations"] + 192
    assert st1["skipped"] == st0["skipped"] + 15 and st1["calls"] == st0["calls"] + 1


# ------------------------------------------------------------------ 6. fan_out()
def test_fan_out_api(engine_factory, oracle):
    """fan_out(pkts, transformers): 5 RawPackets, one of them None, times 3
    transformers, against each transformer's own transform() of copies on a
    twin engine; and doWrite's exclusion."""
    e1, e2 = make_engine(engine_factory), make_engine(engine_factory)
    peers = [Peer([e1, e2], RTP, name, seed()) for name in ("AES_CM_128_HMAC_SHA1_80", "AEAD_AES_256_GCM",
                                                            "F8_128_HMAC_SHA1_80")]
    raw = [rtp(0x6000 + (i & 1), 30 + i, 50 + 13 * i) for i in range(5)]
    pkts = [RawPacket(b"\x00" * 3 + r, 3, len(r)) if i != 2 else None for i, r in enumerate(raw)]
    before = [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts]
    out = fan_out(pkts, [p.e[0] for p in peers])
    assert [None if p is None else (bytes(p.buffer), p.offset, p.length) for p in pkts] == before
    assert len(out) == 3
    for k, p in enumerate(peers):
        copies = [None if q is None else RawPacket(bytes(q.buffer), q.offset, q.length) for q in pkts]
        want = p.e[1].transform(copies)
        assert len(out[k]) == 5 and out[k][2] is None and want[2] is None
        for i in (0, 1, 3, 4):
            assert out[k][i].data() == want[i].data(), (k, i)
            assert out[k][i].length == len(raw[i]) + (16 if p.gcm else 10)
            for key in KEYS_RTP:
                ssrc = 0x6000 + (i & 1)
                assert e1.context_state(p.e[0], ssrc)[key] == e2.context_state(p.e[1], ssrc)[key]
    # the packet's own stream is passed over
    more = [RawPacket(rtp(0x6000, 90 + i, 64)) for i in range(2)]
    out = fan_out(more, [p.e[0] for p in peers], exclusion=[peers[0].e[0], None])
    assert out[0][0] is None and out[0][1] is not None and all(out[k][i] is not None for k in (1, 2) for i in (0, 1))
