"""CPU: the packet-shape grids of tests/shapes.py -- what they cover, and the C
oracle against the independent Python restatement (oracle/pyref.py) on them, in
the manner of test_oracle_crosscheck.py.

tests/test_packet_shapes.py holds the engine to the oracle on these grids, so
the oracle's answers are first held to pyref's here: protect, shapes.tamper,
unprotect, for each cipher / MAC pair that pyref restates; statuses, lengths
and the whole segment bit for bit.  The status counts are pinned: a tamper
cycle or a grid row that turned every packet into a drop would let a kernel
failure hide behind two agreeing errors.
"""
from collections import Counter

import numpy as np
import pytest

import shapes
from libjitsi_amd import profile_policies, synth
from test_oracle_crosscheck import Pair

OK, DROP_REPLAY, DROP_AUTH, DROP_VERSION, ERR_MALFORMED, DROP_INVALID, NOT_PROCESSED = 0, 1, 2, 3, 6, 7, 8
PROFILES = ("AES_CM_128_HMAC_SHA1_80", "AES_CM_128_HMAC_SHA1_32", "F8_128_HMAC_SHA1_80",
            "AES_CM_128_SKEIN_64", "NULL_HMAC_SHA1_80")
SEED = 0x5A9E


def tup(p):
    return (p.encType, p.encKeyLength, p.authType, p.authKeyLength, p.authTagLength, p.saltKeyLength)


def pair(oracle, profile, kind, key_seed):
    P = Pair(oracle)
    (k, s), = synth.keys(key_seed, 1)
    pols = [tup(p) for p in profile_policies(profile)]
    return P, P.transformer(kind, P.factory(True, k, s, *pols)), P.transformer(kind, P.factory(False, k, s, *pols))


def counts(st):
    return dict(Counter(int(s) for s in st))


# ------------------------------------------------------------ 1. the grids
def test_rtp_grid_coverage():
    b = shapes.rtp_grid(SEED)
    assert b.n == 888 == shapes.RTP_N
    hdr, pay = b.meta["header"], b.meta["payload"]
    assert np.array_equal(hdr + pay, b.length)
    assert sorted(set(hdr.tolist())) == sorted({shapes.header_len(*s) for s in shapes.HEADER_SHAPES})
    assert hdr.min() == 12 and hdr.max() == 92
    assert {int(h) % 16 for h in hdr} == {0, 4, 8, 12}  # every payload start class
    for h in sorted(set(hdr.tolist())):
        p = pay[hdr == h]
        assert {(h + int(x) + 4) % 64 for x in p} == set(range(64)), h  # MAC input: packet + ROC
        assert {int(x) % 32 for x in p} == set(range(32)), h
        assert 0 in p and 1 in p and 1188 in p
    assert len(set(b.ssrc.tolist())) == 11
    for s in set(b.ssrc.tolist()):  # every context crosses the ROC wrap
        q = b.seq[b.ssrc == s]
        assert q.max() > 65500 and q.min() < 100
    o = b.off.astype(np.int64)
    assert np.array_equal((b.seg[o] & 0x20) != 0, np.arange(b.n) % 7 == 0)
    assert np.array_equal((b.seg[o + 1] & 0x80) != 0, np.arange(b.n) % 5 == 0)
    assert (b.off % 16 == 0).all() and (b.cap >= b.length + 16).all()
    big = shapes.rtp_grid(SEED, reps=10)
    assert big.n == 8880 and len(set(big.ssrc.tolist())) == 110
    assert np.array_equal(big.length[:888], b.length) and np.array_equal(big.ssrc[:888], b.ssrc)
    assert not np.array_equal(big.seg[int(big.off[888]):int(big.off[888]) + 600], b.seg[:600])  # fresh bytes


def test_rtcp_grid_coverage():
    b = shapes.rtcp_grid(SEED)
    assert b.n == 136
    L = b.length.astype(np.int64)
    assert {int(x) % 4 for x in L} == {0, 1, 2, 3}
    assert {(int(x) + 4) % 64 for x in L if x >= 12} == set(range(64))  # MAC input: packet + index word
    assert {int(x) for x in L if x < 12} == {8, 9, 10, 11}
    assert {1187, 1188, 1189, 1190} <= set(L.tolist())
    o = b.off.astype(np.int64)
    assert (b.seg[o] == 0x80).all() and set(b.seg[o + 1].tolist()) == {200, 201, 202, 203, 204}
    assert len(set(b.ssrc.tolist())) == 7


def test_quirk_grid_coverage():
    """Header minus packet length: the header overshoots the packet by every
    word count 0..8 but 7 (no length of the list lies 28 short of a 72- or
    80-byte header), comes out shorter than 12 bytes and negative (the field
    read as a signed number), and the reference throws where the field lies
    past the buffer."""
    from oracle import pyref
    b = shapes.quirk_grid(SEED)
    assert b.n == 144
    hs, gaps, throws = set(), set(), 0
    for i in range(b.n):
        buf = b.seg[b.off[i]:b.off[i] + b.cap[i]].tobytes()
        try:
            h = pyref.header_len(buf, int(b.cap[i]))
        except pyref.Throw:
            throws += 1
            continue
        hs.add(h)
        gaps.add(int(b.length[i]) - h)
    assert {-32, -24, -20, -16, -12, -8, -4, 0, 4} <= gaps
    assert any(h < 0 for h in hs) and any(0 <= h < 12 for h in hs) and 0 in hs
    assert throws >= 4


def test_tamper_cycle():
    b = shapes.rtp_grid(SEED)
    pos = shapes.tamper_positions(b.length)
    assert sorted(pos) == list(range(0, b.n, 3))
    t = shapes.tamper(b, b.length)
    d = np.nonzero(t.seg != b.seg)[0]
    assert len(d) == len(pos) and set((t.seg[d] ^ b.seg[d]).tolist()) == {0x10}
    assert {p for p in pos.values()} >= {1, 5, 12}
    assert sum(1 for i, p in pos.items() if p == int(b.length[i]) - 1) >= 40


# ------------------------------------------- 2. the oracle against pyref
def round_trip(oracle, profile, kind, b, abort=True):
    P, snd, rcv = pair(oracle, profile, kind, 77)
    pb, st = P.run(snd, False, b, abort=abort)
    tb = shapes.tamper(pb, pb.length)
    ub, st2 = P.run(rcv, True, tb, abort=abort)
    return b, pb, st, ub, st2


@pytest.mark.parametrize("profile", PROFILES)
def test_rtp_grid(oracle, profile):
    """All 888 protected; after tamper 592 accepted and restored, 296 refused."""
    b, pb, st, ub, st2 = round_trip(oracle, profile, 0, shapes.rtp_grid(SEED))
    assert counts(st) == {OK: 888}
    assert counts(st2) == {OK: 592, DROP_AUTH: 296}
    assert (st2 == OK).sum() * 3 >= 2 * b.n
    assert np.array_equal(np.nonzero(st2 == DROP_AUTH)[0], np.arange(0, b.n, 3))
    for i in np.nonzero(st2 == OK)[0]:
        assert ub.length[i] == b.length[i] and ub.packet(i) == b.packet(i)


@pytest.mark.parametrize("profile", PROFILES)
def test_rtcp_grid(oracle, profile):
    """132 protected, the four lengths below 12 invalid.  After tamper the
    ciphered profiles accept 88 and refuse 44.  A NULL-cipher sender writes
    index word 0 into every packet (SRTCPCryptoContext: the index is sent only
    with the E bit), so the receiver takes each SSRC's first intact packet and
    calls the rest replays: pinned apart, and outside the two-thirds rule."""
    b, pb, st, ub, st2 = round_trip(oracle, profile, 1, shapes.rtcp_grid(SEED))
    assert counts(st) == {OK: 132, DROP_INVALID: 4}
    if profile.startswith("NULL"):
        assert counts(st2) == {OK: 7, DROP_AUTH: 9, DROP_REPLAY: 116, DROP_INVALID: 4}
        return
    assert counts(st2) == {OK: 88, DROP_AUTH: 44, DROP_INVALID: 4}
    assert (st2 == OK).sum() * 3 >= 2 * (b.n - 4)
    for i in np.nonzero(st2 == OK)[0]:
        assert ub.length[i] == b.length[i] and ub.packet(i) == b.packet(i)


# what the two references agree on for quirk_grid(SEED): (protect, unprotect)
_CM_EACH = ({OK: 62, ERR_MALFORMED: 82}, {OK: 13, DROP_AUTH: 99, DROP_VERSION: 11, ERR_MALFORMED: 21})
_CM_ABORT = ({ERR_MALFORMED: 1, NOT_PROCESSED: 143}, {DROP_AUTH: 144})
QUIRK_EACH = {
    "AES_CM_128_HMAC_SHA1_80": _CM_EACH, "AES_CM_128_HMAC_SHA1_32": _CM_EACH, "AES_CM_128_SKEIN_64": _CM_EACH,
    "F8_128_HMAC_SHA1_80": ({OK: 108, ERR_MALFORMED: 36},
                            {OK: 44, DROP_AUTH: 70, DROP_VERSION: 9, ERR_MALFORMED: 21}),
    "NULL_HMAC_SHA1_80": ({OK: 144}, {OK: 96, DROP_AUTH: 48}),  # no cipher: the header is never walked
}
QUIRK_ABORT = {
    "AES_CM_128_HMAC_SHA1_80": _CM_ABORT, "AES_CM_128_HMAC_SHA1_32": _CM_ABORT, "AES_CM_128_SKEIN_64": _CM_ABORT,
    # F8 loops over a negative length zero times: the first row passes, the second throws
    "F8_128_HMAC_SHA1_80": ({OK: 16, ERR_MALFORMED: 1, NOT_PROCESSED: 127}, {OK: 10, DROP_AUTH: 134}),
    "NULL_HMAC_SHA1_80": QUIRK_EACH["NULL_HMAC_SHA1_80"],
}


@pytest.mark.parametrize("profile", PROFILES)
def test_quirk_grid_each(oracle, profile):
    """Every packet on its own (abort-on-throw off).  AES-CM: 62 protected and
    82 thrown; of the 144 sent on, 13 accepted, 99 refused by the tag check
    (the 48 tampered ones and those protect threw on, which carry no tag), 11
    with their version bits ciphered away (a header of 0 bytes), 21 thrown."""
    b, pb, st, ub, st2 = round_trip(oracle, profile, 0, shapes.quirk_grid(SEED), abort=False)
    assert (counts(st), counts(st2)) == QUIRK_EACH[profile]


@pytest.mark.parametrize("profile", PROFILES)
def test_quirk_grid_abort(oracle, profile):
    """Abort-on-throw: under AES-CM the first packet (CC = 15 in 12 bytes)
    throws, and the transformer's other 143 are not processed."""
    b, pb, st, ub, st2 = round_trip(oracle, profile, 0, shapes.quirk_grid(SEED), abort=True)
    assert (counts(st), counts(st2)) == QUIRK_ABORT[profile]
    if not profile.startswith("NULL"):  # after the first throw, nothing else
        first = st.tolist().index(ERR_MALFORMED)
        assert (st[first + 1:] == NOT_PROCESSED).all()
