"""The RFC 7714 AES-GCM profiles through the engine's packet path (behind
srtp_engine_enable_aead): k_parse, the sort, k_unprotect / k_protect on their
NULL / NULL path, k_gcm's verify / decipher / seal passes and the walk's GCM
instances.  Every bundle is run through tests/gcm_ref.py on the same bytes
(gcm_ref sends non-GCM contexts to oracle/pyref.py) and statuses, lengths,
every byte of the segment -- the filler between packets included -- and each
touched context's state must agree.  gcm_ref hashes bit by bit in Python, so
payloads stay short and bundles at a few hundred packets; the route test's
large bundles check the unprotect direction against the plaintext they
started from instead (and the state against the reference sender's)."""
import json
import os

import numpy as np
import pytest

import gcm_ref as G
from libjitsi_amd import (SRTCPTransformer, SRTPContextFactory, SRTPDispatcher, SRTPPolicy, SRTPTransformer,
                          profile_policies)
from libjitsi_amd import _native as N
from libjitsi_amd import dtls

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcm_rfc7714.json")
LONG_MIN = 256   # srtp_kernels.h kLongMin: chains from here on are the chain pass's (not GCM ones)
WALK_SPAN = 256  # records per walk tile
RTP, RTCP = 0, 1
KEYS_RTP = ("roc", "s_l", "seq_num_set", "guessed_roc", "replay_window")
KEYS_RTCP = ("sent_index", "received_index", "replay_window")
FILL = 0xA5


def tup(p: SRTPPolicy):
    return (p.encType, p.encKeyLength, p.authType, p.authKeyLength, p.authTagLength, p.saltKeyLength)


GCM128, GCM256 = G.policy(16), G.policy(32)
P80 = tuple(tup(p) for p in profile_policies("AES_CM_128_HMAC_SHA1_80"))


class F:
    """A factory in the reference and in the engine."""

    def __init__(self, eng, sender, mk, ms, srtp, srtcp=None):
        srtcp = srtcp or srtp
        self.r = G.Factory(sender, mk, ms, srtp, srtcp)
        self.e = SRTPContextFactory(sender, mk, ms, SRTPPolicy(*srtp), SRTPPolicy(*srtcp), engine=eng)

    def close(self):
        self.r.close()
        self.e.close()


class T:
    def __init__(self, kind, fwd: F, rev: F = None):
        rev = rev or fwd
        self.kind = kind
        self.r = G.Transformer(kind, fwd.r, rev.r)
        self.e = (SRTPTransformer if kind == RTP else SRTCPTransformer)(fwd.e, rev.e)
        self.tid = self.e.tid


def keys(seed, klen=16, slen=12):
    return G.payload(klen, 1000 + seed), G.payload(slen, 2000 + seed)


def pack(pkts, room=20, caps=None):
    """gcm_ref.pack, with the bytes behind each packet (its room and the
    padding up to the next region) set to a filler that must survive."""
    seg, off, ln, cap = G.pack(pkts, room, caps)
    for i, p in enumerate(pkts):
        a = int(off[i]) + min(len(p), (int(cap[i]) + 15) & ~15)
        b = int(off[i + 1]) if i + 1 < len(pkts) else len(seg)
        seg[a:b] = FILL
    return seg, off, ln, cap


def ssrc_of(kind, seg, o):
    so = 8 if kind == RTP else 4
    return int.from_bytes(seg[o + so:o + so + 4].tobytes(), "big")


def run(eng, ts, reverse, seg, off, ln, cap, flags=None, abort=True, transform=None):
    """One bundle through gcm_ref and the engine; everything must agree.
    Returns the engine's (seg, len, status)."""
    n = len(off)
    per = list(ts) if isinstance(ts, (list, tuple)) else [ts] * n
    seg_r, ln_r = seg.copy(), ln.copy()
    seg_e, ln_e = seg.copy(), ln.copy()
    st_r = G.process([t.r for t in per], reverse, seg_r, off, ln_r, cap, flags, abort)
    tids = np.array([t.tid for t in per], np.int32)
    st_e = (transform or eng.transform_host)(reverse, tids, seg_e, off, ln_e, cap, flags)
    assert st_e.tolist() == st_r.tolist(), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(st_e, st_r)) if a != b][:8]
    assert ln_e.tolist() == ln_r.tolist(), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(ln_e, ln_r)) if a != b][:8]
    if not np.array_equal(seg_e, seg_r):
        d = np.nonzero(seg_e != seg_r)[0]
        pk = np.searchsorted(off.astype(np.int64), d[:4], side="right") - 1
        raise AssertionError(f"segment differs at {d[:4].tolist()} (packets {pk.tolist()}, status "
                             f"{st_r[pk].tolist()}, len in {ln[pk].tolist()}); {len(d)} bytes")
    check_states(eng, per, seg, off, ln)
    return seg_e, ln_e, st_e


def check_states(eng, per, seg, off, ln):
    seen = set()
    for i, t in enumerate(per):
        if ln[i] < 12:
            continue
        ssrc = ssrc_of(t.kind, seg, int(off[i]))
        if (t.tid, ssrc) in seen:
            continue
        seen.add((t.tid, ssrc))
        sr, se = t.r.state(ssrc), eng.context_state(t.e, ssrc)
        assert (sr is None) == (se is None), (hex(ssrc), sr, se)
        if sr is not None:
            for k in (KEYS_RTP if t.kind == RTP else KEYS_RTCP):
                assert int(se[k]) == int(sr[k]), (hex(ssrc), k, sr, se)


def ref_protect(t_r, pkts, room=20):
    """pkts sealed by the reference sender (the engine's input for an unprotect)."""
    seg, off, ln, cap = G.pack(pkts, room)
    st = G.process(t_r, False, seg, off, ln, cap)
    assert st.tolist() == [0] * len(pkts)
    return [seg[off[i]:off[i] + ln[i]].tobytes() for i in range(len(pkts))]


def make_engine(engine_factory, **kw):
    e = engine_factory(max_contexts=1 << 15, max_factories=256, max_transformers=1024, **kw)
    e.enable_aead()
    return e


@pytest.fixture(scope="module")
def eng(engine_factory):
    return make_engine(engine_factory)


@pytest.fixture(scope="module")
def eng_noabort(engine_factory):
    return make_engine(engine_factory, abort_on_error=False)


def sender_receiver(eng, kind, pol, seed):
    mk, ms = keys(seed, pol[1])
    f = F(eng, True, mk, ms, pol)
    return T(kind, f), T(kind, f)


# ------------------------------------------------------------------ 1. golden
def test_golden(eng):
    """OpenSSL's bytes: protect gives the fixture's `out`, unprotect `in`;
    SRTP and SRTCP, both key sizes."""
    with open(GOLDEN) as fh:
        streams = json.load(fh)["streams"]
    seen = set()
    for s in streams:
        key, salt, pol = bytes.fromhex(s["key"]), bytes.fromhex(s["salt"]), tuple(s["policy"])
        seen.add((s["kind"], pol[1]))
        f = F(eng, True, key, salt, pol)
        snd, rcv = T(s["kind"], f), T(s["kind"], f)
        ins = [bytes.fromhex(p["in"]) for p in s["packets"]]
        outs = [bytes.fromhex(p["out"]) for p in s["packets"]]
        seg, off, ln, cap = pack(ins)
        seg2, ln2, st = run(eng, snd, False, seg, off, ln, cap)
        assert st.tolist() == [0] * len(ins)
        for i, want in enumerate(outs):
            assert seg2[off[i]:off[i] + ln2[i]].tobytes() == want, (s["kind"], i)
        seg3, ln3, st = run(eng, rcv, True, seg2, off, ln2, cap)
        assert st.tolist() == [0] * len(ins)
        for i, want in enumerate(ins):
            assert seg3[off[i]:off[i] + ln3[i]].tobytes() == want
    assert seen == {(0, 16), (0, 32), (1, 16), (1, 32)}


# ----------------------------------------------------------------- 2. lengths
@pytest.mark.parametrize("pol", [GCM128, GCM256], ids=["128", "256"])
def test_lengths(eng, pol):
    """Every payload length around the block and pair boundaries, the header
    shapes (data starting 12, 16, 20, 28 and 36 bytes into the packet), SRTCP
    bodies; protect, then unprotect.  Packet regions are 16-byte aligned, as
    the engine requires of every profile (srtp_transform_host refuses others):
    odd packet offsets exist only in the stateless batch (test_gcm_device.py)."""
    snd, rcv = sender_receiver(eng, RTP, pol, 20 + pol[1])
    pk, seq = [], 100
    for plen in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 200):
        for csrcs, ext in ((0, -1), (2, -1), (0, 0), (0, 3), (2, 3)):
            pk.append(G.rtp_packet(0x1000 + csrcs, seq, G.payload(plen, seq), csrcs=csrcs, ext_words=ext))
            seq += 1
    seg, off, ln, cap = pack(pk)
    seg2, ln2, st = run(eng, snd, False, seg, off, ln, cap)
    assert st.tolist() == [0] * len(pk) and (ln2 == ln + 16).all()
    seg3, ln3, st = run(eng, rcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * len(pk) and (ln3 == ln).all()
    for i, p in enumerate(pk):
        assert seg3[off[i]:off[i] + ln3[i]].tobytes() == p
    csnd, crcv = sender_receiver(eng, RTCP, pol, 30 + pol[1])
    pk = [G.rtcp_packet(0x2000 + (i & 1), bytes(4) + G.payload(n, i)) for i, n in enumerate((0, 4, 20, 36, 1, 17))]
    seg, off, ln, cap = pack(pk)
    seg2, ln2, st = run(eng, csnd, False, seg, off, ln, cap)
    assert st.tolist() == [0] * len(pk) and (ln2 == ln + 20).all()
    seg3, ln3, st = run(eng, crcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * len(pk) and (ln3 == ln).all()


# ----------------------------------------------------------- 3. reject shapes
def _raw_rtp(ssrc, seq, b0, rest, total):
    p = bytearray(bytes([b0, 96]) + seq.to_bytes(2, "big") + bytes(4) + ssrc.to_bytes(4, "big") + rest)
    p += G.payload(max(0, total - len(p)), seq)
    return bytes(p[:total])


@pytest.mark.parametrize("abort", [False, True], ids=["each", "abort"])
def test_reject_shapes(eng, eng_noabort, abort):
    """The shapes that end a packet before any cipher work, one bundle each
    way, with abort_on_error off and on (then the rest of that transformer's
    array answers NOT_PROCESSED); the 8- and 11-byte packets also as
    one-packet bundles -- an 8-byte SRTCP protect is where an earlier build
    of this path faulted."""
    e = eng if abort else eng_noabort
    ext_past = lambda s, q: _raw_rtp(s, q, 0x90, b"\xbe\xde" + (50).to_bytes(2, "big"), 40)
    ext_neg = lambda s, q: _raw_rtp(s, q, 0x90, b"\xbe\xde" + (-5 & 0xFFFF).to_bytes(2, "big"), 40)
    for kind in (RTP, RTCP):
        for L in (8, 11):
            for reverse in (False, True):
                t, _ = sender_receiver(e, kind, GCM128, 40 + L)
                seg, off, ln, cap = pack([bytes([0x80, 200, 0, 1]) + G.payload(L - 4, L)], room=24)
                _, _, st = run(e, t, reverse, seg, off, ln, cap, abort=abort)
                assert st.tolist() == [7]
    # protect: one transformer per throwing shape, good packets before and after
    mk, ms = keys(41)
    f = F(e, True, mk, ms, GCM128)
    closed = F(e, True, *keys(42), GCM128)
    ts = [T(RTP, f) for _ in range(3)] + [T(RTCP, f), T(RTP, closed), T(RTCP, closed)]
    closed.close()
    good = lambda s, q: G.rtp_packet(s, q, G.payload(20, q))
    cgood = lambda s, i: G.rtcp_packet(s, G.payload(12, i))
    items = [  # (transformer, packet, cap or None)
        (ts[0], good(1, 1), None), (ts[0], bytes(8), None), (ts[0], ext_past(1, 2), None), (ts[0], good(1, 3), None),
        (ts[1], good(2, 1), None), (ts[1], ext_neg(2, 2), None), (ts[1], good(2, 3), None),
        (ts[2], good(3, 1), len(good(3, 1)) + 15), (ts[2], bytes(11), None), (ts[2], good(3, 2), None),
        (ts[2], _raw_rtp(3, 3, 0x9F, b"", 20), 20 + 16),
        (ts[3], cgood(4, 0), len(cgood(4, 0)) + 19), (ts[3], bytes(8), None), (ts[3], cgood(4, 1), None),
        (ts[4], good(5, 1), None), (ts[5], cgood(6, 0), None),
    ]
    seg, off, ln, cap = pack([p for _, p, _ in items], caps=[c or len(p) + 24 for _, p, c in items])
    _, _, st = run(e, [t for t, _, _ in items], False, seg, off, ln, cap, abort=abort)
    assert st[1] == 7 and st[2] == 6 and st[5] == 6 and st[7] == 5 and st[8] == 7 and st[10] == 6
    assert st[11] == 5 and st[12] == 7 and st[14] == 4 and st[15] == 4
    assert st[3] == (8 if abort else 0) and st[6] == (8 if abort else 0) and st[13] == 0
    # unprotect
    snd, snd_c = T(RTP, f), T(RTCP, f)
    sealed = ref_protect(snd.r, [good(7, q) for q in range(1, 7)])
    csealed = ref_protect(snd_c.r, [cgood(8, i) for i in range(4)])
    rs = [T(RTP, f) for _ in range(3)] + [T(RTCP, f), T(RTCP, f), T(RTP, closed), T(RTCP, closed)]
    items = [
        (rs[0], sealed[0]), (rs[0], bytes(8)), (rs[0], good(7, 50)[:20]),  # L - 16 < h: DROP_AUTH, length 4
        (rs[0], ext_past(7, 51)), (rs[0], ext_neg(7, 52)), (rs[0], sealed[1]),
        (rs[1], sealed[2]), (rs[1], _raw_rtp(7, 53, 0x9F, b"", 20)), (rs[1], sealed[3]),
        (rs[2], bytes(11)), (rs[2], sealed[4]),
    ]
    items += [(rs[3], csealed[0])] + [(rs[3], cgood(8, 9)[:12] + bytes(L - 12)) for L in (20, 23, 27)]
    items += [(rs[3], csealed[1]), (rs[3], cgood(8, 9)[:12] + bytes(3)), (rs[3], csealed[2])]
    items += [(rs[4], bytes([0x80, 200, 0, 1]) + G.payload(L - 4, L)) for L in (12, 19)] + [(rs[4], csealed[3])]
    items += [(rs[5], sealed[5]), (rs[6], csealed[0])]
    seg, off, ln, cap = pack([p for _, p in items], room=8)
    _, ln2, st = run(e, [t for t, _ in items], True, seg, off, ln, cap, abort=abort)
    assert st[:5].tolist() == [0, 7, 2, 2, 6] and ln2[2] == 4 and st[5] == (8 if abort else 0)
    assert st[7] == 6 and st[9] == 7 and st[10] == 0
    assert st[12:15].tolist() == [2, 2, 2] and ln2[12:15].tolist() == [0, 3, 7]
    assert st[16] == 6 and st[17] == (8 if abort else 0) and st[18] == 6 and st[-2:].tolist() == [4, 4]


# --------------------------------------------------------------- 4. tampering
def test_tampering(eng):
    """One flipped bit in the header, the ciphertext, the tag, SRTCP's index
    word: DROP_AUTH, the packet byte for byte as received, the right length;
    a later good packet of the stream is still accepted."""
    for kind, pol in ((RTP, GCM128), (RTCP, GCM256)):
        snd, rcv = sender_receiver(eng, kind, pol, 50 + kind)
        if kind == RTP:
            pk = [G.rtp_packet(0x77, 10 + i, G.payload(40, i), ext_words=1) for i in range(6)]
            spots = (1, 24, -3, 30)  # header, ciphertext, tag, ciphertext
        else:
            pk = [G.rtcp_packet(0x78, G.payload(36, i)) for i in range(6)]
            spots = (1, 20, -9, -2)  # header, ciphertext, tag, the E|index word
        sealed = ref_protect(snd.r, pk)
        bad = []
        for i, at in enumerate(spots):
            b = bytearray(sealed[i])
            b[at] ^= 1 << (i + 1)
            bad.append(bytes(b))
        items = bad + sealed[4:]
        seg, off, ln, cap = pack(items, room=4)
        seg2, ln2, st = run(eng, rcv, True, seg, off, ln, cap)
        assert st.tolist() == [2, 2, 2, 2, 0, 0]
        trailer = 16 if kind == RTP else 20
        assert ln2.tolist() == [len(p) - trailer for p in items]
        for i in range(4):
            assert seg2[off[i]:off[i] + len(bad[i])].tobytes() == bad[i]
        # the forged packets' originals are still fresh: accepted now
        seg, off, ln, cap = pack(sealed[:4], room=4)
        _, _, st = run(eng, rcv, True, seg, off, ln, cap)
        assert st.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------- 5. state
def _stream(ssrc, seqs, plen=16):
    return [G.rtp_packet(ssrc, q & 0xFFFF, G.payload(plen, q)) for q in seqs]


def test_state(eng):
    """Replay and ROC state: duplicates and reordering inside and across
    bundles, replays older than 64, the wrap 65534 -> 2 inside a bundle and
    across two, a walk ROC that differs from the verify pass's guess (the
    one-block re-check runs, and still refuses a forged packet), and the
    DISCARD / SILENCE flags (verified, state advanced, not deciphered)."""
    snd, rcv = sender_receiver(eng, RTP, GCM128, 60)
    seqs = [100, 101, 101, 103, 102, 102, 110, 109, 180, 100, 115, 116, 181]
    sealed = ref_protect(snd.r, _stream(0xA1, sorted(set(seqs))))
    by = dict(zip(sorted(set(seqs)), sealed))
    seg, off, ln, cap = pack([by[q] for q in seqs], room=4)
    _, _, st = run(eng, rcv, True, seg, off, ln, cap)
    assert st[2] == 1 and st[5] == 1 and st[9] == 1 and st[10] == 1  # duplicates; 115 is 65 behind 180
    assert st[:2].tolist() == [0, 0] and st[3:5].tolist() == [0, 0] and st[6:9].tolist() == [0, 0, 0]
    seg, off, ln, cap = pack([by[q] for q in (181, 116, 110, 180)], room=4)  # across bundles: all replays
    _, _, st = run(eng, rcv, True, seg, off, ln, cap)
    assert st.tolist() == [1, 1, 1, 1]
    # the wrap inside one bundle, and across two
    snd, rcv = sender_receiver(eng, RTP, GCM256, 61)
    q1 = [65533, 65534, 2 + 65536, 3 + 65536, 65535, 1 + 65536]
    sealed = ref_protect(snd.r, _stream(0xA2, sorted(q1)))
    by = dict(zip(sorted(q1), sealed))
    seg, off, ln, cap = pack([by[q] for q in q1], room=4)
    _, _, st = run(eng, rcv, True, seg, off, ln, cap)
    assert st.tolist() == [0] * 6 and eng.context_state(rcv.e, 0xA2)["roc"] == 1
    snd, rcv = sender_receiver(eng, RTP, GCM128, 62)
    a, b = _stream(0xA3, [65530, 65534]), _stream(0xA3, [2 + 65536, 5 + 65536])
    sa, sb = ref_protect(snd.r, a), ref_protect(snd.r, b)
    for part in (sa, sb):
        seg, off, ln, cap = pack(part, room=4)
        _, _, st = run(eng, rcv, True, seg, off, ln, cap)
        assert st.tolist() == [0, 0]
    assert eng.context_state(rcv.e, 0xA3)["roc"] == 1
    # a walk ROC other than the verify pass's guess: s_l moves across the 2^15
    # thresholds inside the bundle (test_roc_guess_overturned_by_walk's shape)
    snd, rcv = sender_receiver(eng, RTP, GCM128, 63)
    c0 = eng.stats()["roc_rechecks"]
    for k, qs in enumerate(([100], [30000, 60000, 10 + 65536, 20 + 65536, 40000, 70 + 65536, 33000],
                            [30000 + 65536, 60000 + 65536, 5 + 131072])):
        order = sorted(range(len(qs)), key=lambda i: qs[i])
        sealed = ref_protect(snd.r, _stream(0xA4, [qs[i] for i in order]))
        items = [None] * len(qs)
        for j, i in enumerate(order):
            items[i] = sealed[j]
        if k == 2:  # the last one's ROC (2) is not the bundle-start guess (1): forge a copy of it
            bad = bytearray(items[2])
            bad[-1] ^= 0x10
            items = [items[0], items[1], bytes(bad), items[2]]
        seg, off, ln, cap = pack(items, room=4)
        _, _, st = run(eng, rcv, True, seg, off, ln, cap)
        if k == 2:
            assert st.tolist() == [0, 0, 2, 0]
    assert eng.stats()["roc_rechecks"] > c0
    # DISCARD / SILENCE
    snd, rcv = sender_receiver(eng, RTP, GCM256, 64)
    sealed = ref_protect(snd.r, _stream(0xA5, range(5, 11), plen=33))
    flags = np.array([0, N.PKT_FLAG_DISCARD, N.PKT_FLAG_SILENCE, 0, N.PKT_FLAG_DISCARD | N.PKT_FLAG_SILENCE, 0], np.uint32)
    seg, off, ln, cap = pack(sealed, room=4)
    seg2, ln2, st = run(eng, rcv, True, seg, off, ln, cap, flags=flags)
    assert st.tolist() == [0] * 6
    for i in (1, 2, 4):  # still ciphertext
        assert seg2[off[i]:off[i] + ln2[i]].tobytes() == sealed[i][:-16]
    assert eng.context_state(rcv.e, 0xA5)["s_l"] == 10
    # SRTCP: duplicates, reordering, an index more than 64 behind
    csnd, crcv = sender_receiver(eng, RTCP, GCM128, 65)
    sealed = ref_protect(csnd.r, [G.rtcp_packet(0xA6, G.payload(20, i)) for i in range(70)])
    order = [0, 2, 1, 1, 69, 3, 4, 68, 69]
    seg, off, ln, cap = pack([sealed[i] for i in order], room=4)
    _, _, st = run(eng, crcv, True, seg, off, ln, cap)
    assert st[3] == 1 and st[8] == 1 and st[:3].tolist() == [0, 0, 0] and st[4] == 0


# ------------------------------------------------------------- 6. SRTCP E = 0
def test_srtcp_e0(eng):
    """RFC 7714 9.3: an unencrypted SRTCP packet, AAD = the packet up to the
    tag || the E|index word; built with gcm_ref.seal."""
    mk, ms = keys(70)
    f = F(eng, True, mk, ms, GCM128)
    rcv = T(RTCP, f)
    enc, salt = G.derive(mk, ms, True)
    rks = G.expand_key(enc)
    pk = []
    for idx, body in ((1, 28), (2, 9), (3, 28)):
        p = G.rtcp_packet(0xE0, G.payload(body, idx))
        wb = idx.to_bytes(4, "big")  # E = 0
        _, tag = G.seal(rks, G.rtcp_iv(salt, p[4:8], idx), p + wb, b"")
        pk.append(p + tag + wb)
    bad = bytearray(pk[2])
    bad[10] ^= 0x40
    pk[2] = bytes(bad)
    seg, off, ln, cap = pack(pk, room=4)
    seg2, ln2, st = run(eng, rcv, True, seg, off, ln, cap)
    assert st.tolist() == [0, 0, 2] and np.array_equal(seg2, seg)  # nothing is ciphered either way
    assert ln2.tolist() == [len(p) - 20 for p in pk]


# ------------------------------------------------------------------ 7. chains
@pytest.mark.parametrize("stall", [False, True], ids=["plain", "forced_stall"])
def test_chains(eng, stall):
    """One SSRC with kLongMin + 5 records, and one whose records span two walk
    tiles (behind 200 other records), beside short streams; again with the
    chain pass's look-back forced to stall.  A GCM chain is walked record by
    record whatever its length."""
    eng.set_debug(N.DEBUG_FORCE_CHAIN_STALL if stall else 0)
    try:
        snd, rcv = sender_receiver(eng, RTP, GCM128, 80 + stall)
        mk, ms = keys(82 + stall, 16, 14)
        fh = F(eng, True, mk, ms, *P80)
        hs, hr = T(RTP, fh), T(RTP, fh)
        n_long = LONG_MIN + 5
        pk = [(snd, rcv, p) for p in _stream(0xC1, range(65400, 65400 + n_long))]
        pk += [(snd, rcv, p) for s in range(40) for p in _stream(0xC200 + s, range(7, 12))]  # 200 records
        pk += [(snd, rcv, p) for p in _stream(0xFFFFFF00, range(1, 1 + WALK_SPAN + 40))]  # sorts last: spans tiles
        pk += [(hs, hr, p) for p in _stream(0xC3, range(50, 50 + n_long), plen=16)]  # an HMAC long chain beside them
        # interleave the streams, each keeping its own (a sender's) order
        by_stream = {}
        for it in pk:
            by_stream.setdefault((it[0].tid, it[2][8:12]), []).append(it)
        slots = [k for k, v in by_stream.items() for _ in v]
        rng = np.random.default_rng(83)
        items = [by_stream[slots[i]].pop(0) for i in rng.permutation(len(slots))]
        seg, off, ln, cap = pack([p for _, _, p in items])
        seg2, ln2, st = run(eng, [s for s, _, _ in items], False, seg, off, ln, cap)
        assert st.tolist() == [0] * len(items)
        seg3, ln3, st = run(eng, [r for _, r, _ in items], True, seg2, off, ln2, cap)
        assert st.tolist() == [0] * len(items) and np.array_equal(ln3, ln)
        assert eng.context_state(rcv.e, 0xC1)["roc"] == 1
    finally:
        eng.set_debug(0)


# ------------------------------------------------------------ 8. mixed engine
def test_mixed_engine(eng):
    """GCM-128, GCM-256, AES_CM_128_HMAC_SHA1_80, F8 and a Skein profile on
    different transformers of one bundle; 70 GCM factories, so that one wave
    meets more than 64 key sets; a factory with a GCM SRTP policy and an HMAC
    SRTCP policy."""
    pairs = []
    for i in range(70):
        pol = GCM128 if i % 2 else GCM256
        pairs.append(sender_receiver(eng, RTP, pol, 100 + i))
    for name in ("AES_CM_128_HMAC_SHA1_80", "F8_128_HMAC_SHA1_80", "AES_CM_128_SKEIN_32"):
        sp, cp = (tup(p) for p in profile_policies(name))
        mk, ms = keys(180 + len(pairs), 16, 14)
        f = F(eng, True, mk, ms, sp, cp)
        pairs.append((T(RTP, f), T(RTP, f)))
    mk, ms = keys(190, 16, 14)
    fm = F(eng, True, mk, ms, GCM128, P80[1])  # GCM SRTP, HMAC SRTCP
    pairs.append((T(RTP, fm), T(RTP, fm)))
    cm = (T(RTCP, fm), T(RTCP, fm))
    fm2 = F(eng, True, *keys(191, 16, 14), P80[0], GCM128)  # and the other way round
    pairs.append((T(RTP, fm2), T(RTP, fm2)))
    cm2 = (T(RTCP, fm2), T(RTCP, fm2))
    items = []
    for rnd in range(2):
        for k, (s, r) in enumerate(pairs):
            items.append((s, r, G.rtp_packet(0xD000 + k, 20 + rnd, G.payload(16 + (k % 5), k + rnd))))
        for k, (s, r) in enumerate((cm, cm2)):
            items.append((s, r, G.rtcp_packet(0xD800 + k, G.payload(16, k + rnd))))
    seg, off, ln, cap = pack([p for _, _, p in items], room=24)
    seg2, ln2, st = run(eng, [s for s, _, _ in items], False, seg, off, ln, cap)
    assert st.tolist() == [0] * len(items)
    seg3, ln3, st = run(eng, [r for _, r, _ in items], True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * len(items) and np.array_equal(ln3, ln)
    for i in range(len(items)):
        assert seg3[off[i]:off[i] + ln[i]].tobytes() == items[i][2]


# --------------------------------------------------------- 9. routes by size
@pytest.mark.parametrize("n", [1, 255, 256, 3000, 9000])
def test_routes_by_bundle_size(eng, n):
    """Bundle sizes on either side of k_small's limit, inside the split path's
    range and past kSmallCtrMax: an engine with a GCM key set runs them all on
    the multi-kernel path (no k_small bundle).  Protect is held to gcm_ref;
    the unprotect of these bundles to the plaintext they started from and to
    the reference sender's state (in-order streams: the receiver's equals it)."""
    snd, rcv = sender_receiver(eng, RTP, GCM128, 200 + (n & 0xFF))
    small0 = eng.stats()["small_bundles"]
    n_ssrc = max(1, n // 25)
    pk = [G.rtp_packet(0xE0000 + (i % n_ssrc), 1 + i // n_ssrc, G.payload(32, i)) for i in range(n)]
    seg, off, ln, cap = pack(pk, room=16)
    seg2, ln2, st = run(eng, snd, False, seg, off, ln, cap)
    assert st.tolist() == [0] * n
    seg3, ln3 = seg2.copy(), ln2.copy()
    st = eng.transform_host(True, rcv.tid, seg3, off, ln3, cap)
    assert st.tolist() == [0] * n and np.array_equal(ln3, ln)
    for i in range(n):
        o = int(off[i])
        assert np.array_equal(seg3[o:o + ln[i]], seg[o:o + ln[i]]), i
        assert np.array_equal(seg3[o + ln[i]:o + int(cap[i])], seg2[o + ln[i]:o + int(cap[i])]), i
    for s in range(n_ssrc):
        sr, se = snd.r.state(0xE0000 + s), eng.context_state(rcv.e, 0xE0000 + s)
        for k in ("roc", "s_l", "seq_num_set", "replay_window"):
            assert int(se[k]) == int(sr[k]), (s, k, sr, se)
    assert eng.stats()["small_bundles"] == small0


# ------------------------------------------------------------------ 10. switch
def test_switch(engine_factory):
    e = engine_factory(max_contexts=4096, max_factories=16, max_transformers=16)
    off_twin = engine_factory(max_contexts=4096, max_factories=16, max_transformers=16)
    mk, ms = keys(300)
    pol = SRTPPolicy(*GCM128)
    with pytest.raises(N.SrtpError, match="SRTP_EPOLICY"):
        SRTPContextFactory(True, mk, ms, pol, pol, engine=e)
    e.enable_aead()
    # on, and no GCM factory: a mixed AES-CM bundle comes out as with the switch off
    k14 = keys(301, 16, 14)
    outs = []
    for x in (e, off_twin):
        f = F(x, True, *k14, *P80)
        s, r = T(RTP, f), T(RTP, f)
        pk = [G.rtp_packet(0x300 + (i % 3), 9 + i, G.payload(10 + 7 * i, i)) for i in range(12)]
        seg, off, ln, cap = pack(pk)
        seg2, ln2, st = run(x, s, False, seg, off, ln, cap)
        seg3, ln3, st3 = run(x, r, True, seg2, off, ln2, cap)
        outs.append((seg2.tobytes(), ln2.tolist(), st.tolist(), seg3.tobytes(), ln3.tolist(), st3.tolist()))
    assert outs[0] == outs[1]
    for bad in ((5, 24, 0, 0, 16, 12), (5, 16, 0, 0, 12, 12), (5, 16, 0, 0, 16, 14), (5, 16, 1, 20, 16, 12),
                (5, 16, 0, 20, 16, 12)):
        with pytest.raises(N.SrtpError, match="SRTP_EPOLICY"):
            SRTPContextFactory(True, bytes(32), bytes(14), SRTPPolicy(*bad), SRTPPolicy(*bad), engine=e)
    f = F(e, True, mk, ms, GCM128)
    snd, rcv = T(RTP, f), T(RTP, f)
    e.enable_aead(False)
    with pytest.raises(N.SrtpError, match="SRTP_EPOLICY"):
        SRTPContextFactory(True, mk, ms, pol, pol, engine=e)
    pk = _stream(0x310, range(3, 9))
    seg, off, ln, cap = pack(pk)
    seg2, ln2, st = run(e, snd, False, seg, off, ln, cap)  # the old factory still transforms
    _, _, st2 = run(e, rcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * 6 and st2.tolist() == [0] * 6


# --------------------------------------------------------- 11. export / import
def test_export_import(engine_factory):
    A, B = make_engine(engine_factory), make_engine(engine_factory)
    mk, ms = keys(400, 32)
    fa, fb = F(A, True, mk, ms, GCM256), F(B, True, mk, ms, GCM256)
    for kind in (RTP, RTCP):
        snd, rcv_a, rcv_b = T(kind, fa), T(kind, fa), T(kind, fb)
        if kind == RTP:
            pk = [p for s in (0x41, 0x42) for p in _stream(s, range(65500, 65560))]
        else:
            pk = [G.rtcp_packet(0x43 + (i >= 60), G.payload(16, i)) for i in range(120)]
        sealed = ref_protect(snd.r, pk)
        first, later = sealed[:40] + sealed[60:100], sealed[40:60] + sealed[100:]
        seg, off, ln, cap = pack(first, room=4)
        run(A, rcv_a, True, seg, off, ln, cap)
        ex = A.export_contexts(rcv_a.e)
        assert len(ex) == 2
        for ssrc, st in ex.items():
            sr = rcv_a.r.state(ssrc)
            for k in (KEYS_RTP if kind == RTP else KEYS_RTCP):
                assert int(st[k]) == int(sr[k])
            B.import_context(rcv_b.e, ssrc, st, forward=False)
        rcv_b.r.ctx = rcv_a.r.ctx  # the reference's contexts move with the streams
        items = first[:3] + later + first[-2:]  # replays of what only A saw, new traffic
        seg, off, ln, cap = pack(items, room=4)
        _, _, st = run(B, rcv_b, True, seg, off, ln, cap)
        assert st[:3].tolist() == [1, 1, 1] and st[3:-2].tolist() == [0] * len(later)
        if kind == RTP:  # (the reference's SRTCP window update shifts on old indices: no such promise there)
            assert st[-2:].tolist() == [1, 1]


# -------------------------------------------------------------- 12. dispatcher
def test_dispatcher():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    d = SRTPDispatcher([0, 0], max_contexts=4096, max_factories=16, max_transformers=16)
    try:
        mk, ms = keys(500)
        pol = SRTPPolicy(*GCM128)
        with pytest.raises(N.SrtpError, match="SRTP_EPOLICY"):
            SRTPContextFactory(True, mk, ms, pol, pol, engine=d)
        d.enable_aead()
        f = F(d, True, mk, ms, GCM128)
        ts = {k: (T(k, f), T(k, f)) for k in (RTP, RTCP)}
        items = []
        for i in range(48):
            items.append((RTP, G.rtp_packet(0x500 + (i % 8), 3 + i // 8, G.payload(16 + i % 7, i))))
            if i % 4 == 0:
                items.append((RTCP, G.rtcp_packet(0x580 + (i % 8), G.payload(12, i))))
        assert len({d.shard_of(0x500 + s) for s in range(8)}) == 2  # both shards take part
        seg, off, ln, cap = pack([p for _, p in items], room=24)
        seg2, ln2, st = run(d, [ts[k][0] for k, _ in items], False, seg, off, ln, cap, transform=d.transform_host)
        assert st.tolist() == [0] * len(items)
        bad = bytearray(seg2)
        bad[int(off[5]) + 14] ^= 2
        seg2 = np.frombuffer(bytes(bad), np.uint8).copy()
        _, ln3, st = run(d, [ts[k][1] for k, _ in items], True, seg2, off, ln2, cap, transform=d.transform_host)
        assert st.tolist() == [0] * 5 + [2] + [0] * (len(items) - 6)
    finally:
        d.close()


# -------------------------------------------------------------------- 13. DTLS
@pytest.mark.parametrize("pid", dtls.AEAD_PROFILES)
def test_dtls_aead_profiles(eng, pid):
    """profile_keys(7 | 8, aead=True) from exported keying material into a
    factory pair per endpoint; both directions round-trip a bundle."""
    k0 = dtls.profile_keys(pid, aead=True)
    km = dtls.export_keying_material(G.payload(48, pid), G.payload(32, 1), G.payload(32, 2),
                                     k0["keying_material_len"], prf=dtls.PRF_SHA256)
    k = dtls.profile_keys(pid, km, aead=True)
    sp, cp = tup(k["srtpPolicy"]), tup(k["srtcpPolicy"])
    assert sp == cp == G.policy(16 if pid == 7 else 32)
    ends = {}
    for is_client in (True, False):
        fc = F(eng, is_client, k["client_key"], k["client_salt"], sp, cp)
        fs = F(eng, not is_client, k["server_key"], k["server_salt"], sp, cp)
        fwd, rev = (fc, fs) if is_client else (fs, fc)
        ends[is_client] = {kind: T(kind, fwd, rev) for kind in (RTP, RTCP)}
    for sender in (True, False):
        for kind in (RTP, RTCP):
            # an SSRC per direction: a transformer keeps one context per SSRC, whichever way it was made
            ssrc = 0x600 + 2 * sender
            pk = [G.rtp_packet(ssrc, 4 + i, G.payload(20, i)) if kind == RTP else G.rtcp_packet(ssrc + 1, G.payload(16, i))
                  for i in range(4)]
            seg, off, ln, cap = pack(pk, room=24)
            seg2, ln2, st = run(eng, ends[sender][kind], False, seg, off, ln, cap)
            seg3, ln3, st3 = run(eng, ends[not sender][kind], True, seg2, off, ln2, cap)
            assert st.tolist() == [0] * 4 and st3.tolist() == [0] * 4 and np.array_equal(ln3, ln)
            for i in range(4):
                assert seg3[off[i]:off[i] + ln[i]].tobytes() == pk[i]
