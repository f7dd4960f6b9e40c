"""Receive with the ssrc-audio-level read on the device
(srtp_transform_device_lvl / _host_lvl, k_audio_level, reverse_transform_levels()).

Equivalence: for each bundle the _lvl call equals the existing call
(transform_device / transform_host, reverse) given flags made on the host by
audio_level_ref -- SsrcTransformEngine.reverseTransform restated -- on a twin
transformer of the same keys: the whole segment, len, status and the contexts'
state bit for bit, and level equal to the reference's.  The bundles mix the
header shapes of audio_level_ref.header_shapes (no X bit, a zero and a negative
length word, the element first, second and last, IDs 1..7 and 8..15, padding,
both two-byte cases, 0, 1, 11 and 15 CSRCs, a data byte at len, version 1,
len < 12) with len > cap, caller SKIP and DISCARD, tampered tags and replays.
Shapes that no SRTP sender makes ("wild": they may throw in SRTP, which aborts
the transformer's later packets) go to a transformer of their own where the
bundle carries one ID per packet, and to the bundle's end where it has one."""
import numpy as np
import pytest

import audio_level_ref as R
from harness import STATE_KEYS_RTP, Twin
from libjitsi_amd import RawPacket, SRTPContextFactory, SRTPTransformer, profile_policies, reverse_transform_levels
from libjitsi_amd import _native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CM, GCM = "AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM"
SKIP, SILENCE, DISCARD = N.PKT_FLAG_SKIP, N.PKT_FLAG_SILENCE, N.PKT_FLAG_DISCARD
LEVELS = (0x7F, 0x0A, 0xFF, 0x00, 0x8A, 0x7E)
N_SSRC = 61
SIZES = (1, 3, 255, 256, 2049)


def up16(v):
    return (int(v) + 15) & ~15


def key_of(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    O.set_check_replay(True)
    return engine_factory(max_contexts=1 << 15, max_factories=256, max_transformers=1024)


@pytest.fixture(scope="module")
def eng_gcm(engine_factory):
    e = engine_factory(max_contexts=1 << 15, max_factories=256, max_transformers=1024)
    e.enable_aead()
    return e


_base = [0x5A000000]


class Keys:
    """One master key: a sender and as many receivers of it as asked for, on one engine."""

    def __init__(self, eng, profile, seed):
        self.eng, self.pols = eng, profile_policies(profile)
        self.mk, self.ms = key_of(seed, 16), key_of(seed + 1, 12 if profile == GCM else 14)
        self.snd = SRTPTransformer(SRTPContextFactory(True, self.mk, self.ms, *self.pols, engine=eng))

    def receiver(self):
        return SRTPTransformer(SRTPContextFactory(False, self.mk, self.ms, *self.pols, engine=self.eng))


class Bundle:
    """n received packets: (seg, off, len, cap), the caller's flags, one ID per packet, which are wild, and
    the reference's (level, flags) of each.  first: the shape the bundle starts its cycle at."""

    def __init__(self, keys, n, first="first", wild_last=False, with_wild=True):
        eng = keys.eng
        _base[0] += 0x1000
        base = _base[0]
        names = [s[0] for s in R.header_shapes()]
        start = names.index(first)
        plain, self.wild, self.eid, self.ssrc = [], [], [], []
        for i in range(n):
            eid, lvl = 1 + (i // 3) % 7, LEVELS[i % len(LEVELS)]
            shapes = R.header_shapes(eid, lvl)
            if not with_wild:
                shapes = [s for s in shapes if not s[2]]
            _, build, wild = shapes[(start + i) % len(shapes)] if with_wild else shapes[i % len(shapes)]
            ssrc, seq = base + i % N_SSRC, 100 + i // N_SSRC
            payload = bytes((7 * i + k) & 0xFF for k in range(20 + (i * 7) % 70))
            plain.append(build(ssrc, seq, payload))
            self.wild.append(wild)
            self.eid.append(eid)
            self.ssrc.append(ssrc)
        if wild_last:  # a throw aborts the transformer's later packets: keep those the wild ones
            order = [i for i in range(n) if not self.wild[i]] + [i for i in range(n) if self.wild[i]]
            plain, self.wild, self.eid, self.ssrc = ([x[i] for i in order] for x in (plain, self.wild, self.eid, self.ssrc))
        self.plain = plain
        self.n = n
        # the sender's work: every packet a sender can make, protected in one bundle
        room = eng.trailer_room
        good = [i for i in range(n) if not self.wild[i]]
        sent = list(plain)
        if good:
            cap = np.array([len(plain[i]) + room for i in good], np.uint32)
            off = np.concatenate(([0], np.cumsum([up16(c) for c in cap])[:-1])).astype(np.uint32)
            ln = np.array([len(plain[i]) for i in good], np.uint32)
            seg = np.zeros(int(off[-1]) + up16(cap[-1]), np.uint8)
            for k, i in enumerate(good):
                seg[off[k]:off[k] + ln[k]] = np.frombuffer(plain[i], np.uint8)
            st = eng.transform_host(False, keys.snd.tid, seg, off, ln, cap)
            assert (st == N.STATUS_OK).all(), [(i, int(x)) for i, x in zip(good, st) if x][:5]
            for k, i in enumerate(good):
                sent[i] = seg[off[k]:off[k] + ln[k]].tobytes()
        self.protected = list(sent)
        # the network's: tampered tags and replays
        self.tampered, self.replayed = set(), set()
        for i in range(n):
            if not self.wild[i] and i % 11 == 5:
                sent[i] = sent[i][:-1] + bytes([sent[i][-1] ^ 0x40])
                self.tampered.add(i)
        for i in range(N_SSRC, n):
            if i % 13 == 7 and not self.wild[i] and not self.wild[i - N_SSRC] and (i - N_SSRC) not in self.tampered \
                    and i not in self.tampered and not wild_last:
                sent[i] = self.protected[i - N_SSRC]  # the same SSRC's earlier packet once more
                self.eid[i] = self.eid[i - N_SSRC]
                self.replayed.add(i)
        self.sent = sent
        self.len = np.array([len(p) for p in sent], np.uint32)
        self.cap = np.array([max(len(p), 1) + (i % 3) * 8 for i, p in enumerate(sent)], np.uint32)
        self.flags = np.zeros(n, np.uint32)
        for i in range(n):
            if n > 3 and i % 17 == 3:
                self.flags[i] = DISCARD
            if n > 3 and i % 19 == 4:
                self.flags[i] |= SKIP
            if n > 3 and i % 23 == 6:
                self.cap[i] = max(len(sent[i]) - 1, 0)  # len > cap: RawPacket.isInvalid
        self.off = np.concatenate(([0], np.cumsum([up16(c) for c in self.cap])[:-1])).astype(np.uint32)
        self.seg = np.full(int(self.off[-1]) + up16(self.cap[-1]), 0xA5, np.uint8)
        for i, p in enumerate(sent):
            k = min(len(p), up16(self.cap[i]))
            self.seg[self.off[i]:self.off[i] + k] = np.frombuffer(p[:k], np.uint8)

    def ids(self, mode):
        """One ID per packet -- its element's, with zeros, other IDs and IDs >= 128 mixed in -- or ID 1 for all."""
        if mode == "scalar":
            return np.full(self.n, 1, np.uint8)
        ids = np.array(self.eid, np.uint8)
        for i in range(self.n):
            if i % 5 == 2:
                ids[i] = 0
            elif i % 7 == 3:
                ids[i] = ids[i] % 7 + 1
            elif i % 29 == 9:
                ids[i] = 200
            elif i % 31 == 11:
                ids[i] |= 8  # 9..15: no one-byte element is read as that
        return ids

    def reference(self, ids):
        """audio_level_ref over every entry: (levels, flags, entries read)."""
        lv, fl, read = np.zeros(self.n, np.int8), np.zeros(self.n, np.uint32), 0
        for i in range(self.n):
            o, ln, cap = int(self.off[i]), int(self.len[i]), int(self.cap[i])
            lv[i], fl[i] = R.reverse_transform(self.seg[o:o + up16(cap)].tobytes(), ln, cap, int(self.flags[i]),
                                               int(ids[i]))
            read += not self.flags[i] & SKIP and 1 <= ids[i] <= 127 and 12 <= ln <= cap
        return lv, fl, read


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_lvl(eng, route, tid, b, ids, mode, flags):
    """The _lvl call: (seg, len, status, level)."""
    ext_ids, ext_id = (ids, 0) if mode == "array" else (None, int(ids[0]) if len(ids) else 0)
    if route == "host":
        seg, ln = b.seg.copy(), b.len.copy()
        st, lv = eng.transform_host_lvl(tid, seg, b.off, ln, b.cap, flags, ext_ids, ext_id)
        return seg, ln, st, lv
    import torch
    seg, ln = dev(b.seg.copy()), dev(b.len.copy())
    st = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    lv = torch.full((b.n,), 99, dtype=torch.int8, device="cuda")
    t = tid if np.isscalar(tid) else dev(tid)
    torch.cuda.synchronize()
    try:
        eng.transform_device_lvl(t, seg, dev(b.off), ln, dev(b.cap), st, lv, None if flags is None else dev(flags),
                                 None if ext_ids is None else dev(ext_ids), ext_id)
    finally:
        eng.sync()
        torch.cuda.synchronize()
    return seg.cpu().numpy(), ln.cpu().numpy().view(np.uint32), st.cpu().numpy(), lv.cpu().numpy()


def run_plain(eng, route, tid, b, flags):
    """The existing call with the flags given: (seg, len, status)."""
    if route == "host":
        seg, ln = b.seg.copy(), b.len.copy()
        st = eng.transform_host(True, tid, seg, b.off, ln, b.cap, flags)
        return seg, ln, st
    import torch
    seg, ln = dev(b.seg.copy()), dev(b.len.copy())
    st = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    t = tid if np.isscalar(tid) else dev(tid)
    torch.cuda.synchronize()
    try:
        eng.transform_device(True, t, seg, dev(b.off), ln, dev(b.cap), st, None if flags is None else dev(flags))
    finally:
        eng.sync()
        torch.cuda.synchronize()
    return seg.cpu().numpy(), ln.cpu().numpy().view(np.uint32), st.cpu().numpy()


def same_states(eng, pairs, ssrcs):
    for ta, tb in pairs:
        for ssrc in sorted(set(ssrcs)):
            sa, sb = eng.context_state(ta, ssrc), eng.context_state(tb, ssrc)
            assert (sa is None) == (sb is None), hex(ssrc)
            if sa is not None:
                assert [sa[k] for k in STATE_KEYS_RTP] == [sb[k] for k in STATE_KEYS_RTP], (hex(ssrc), sa, sb)


def equivalent(keys, b, route, mode, pass_flags=True):
    """The _lvl call on receivers A against the existing call on receivers B with the reference's flags."""
    eng = keys.eng
    ids = b.ids(mode)
    want_lv, want_fl, read = b.reference(ids)
    a_main, a_wild, b_main, b_wild = (keys.receiver() for _ in range(4))
    if mode == "array":  # one transformer ID per packet too: the wild shapes on a transformer of their own
        tid_a = np.array([a_wild.tid if w else a_main.tid for w in b.wild], np.int32)
        tid_b = np.array([b_wild.tid if w else b_main.tid for w in b.wild], np.int32)
    else:
        tid_a, tid_b = a_main.tid, b_main.tid
    flags = b.flags if pass_flags else None
    s0 = eng.audio_level_stats()
    seg, ln, st, lv = run_lvl(eng, route, tid_a, b, ids, mode, flags)
    s1 = eng.audio_level_stats()
    seg_w, ln_w, st_w = run_plain(eng, route, tid_b, b, want_fl)
    assert np.array_equal(lv, want_lv), np.nonzero(lv != want_lv)[0][:10]
    assert np.array_equal(st, st_w), [(int(i), int(st[i]), int(st_w[i])) for i in np.nonzero(st != st_w)[0][:10]]
    assert np.array_equal(ln, ln_w)
    assert np.array_equal(seg, seg_w)
    same_states(eng, [(a_main, b_main), (a_wild, b_wild)], b.ssrc)
    assert s1["calls"] == s0["calls"] + 1
    assert s1["entries_read"] - s0["entries_read"] == read
    assert s1["levels_found"] - s0["levels_found"] == int((want_lv >= 0).sum())
    assert s1["silent"] - s0["silent"] == int((want_lv == 127).sum())
    return st, lv, ln, seg


@pytest.mark.parametrize("mode", ["array", "scalar"])
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_lvl_equals_host_made_flags(eng, n, route, mode):
    """Bundles of 1, 3, 255, 256 and 2049 packets (k_small, the chain, the split
    path; a wave's last partial trip), device and host route, tids and ext_ids
    as arrays (mixed IDs and zeros) and as scalars."""
    keys = Keys(eng, CM, 100 + n)
    b = Bundle(keys, n, wild_last=mode == "scalar")
    st, lv, ln, seg = equivalent(keys, b, route, mode)
    if n >= 255:
        ok = st == N.STATUS_OK
        muted = lv == 127
        assert (ok & muted).sum() > 0 and (ok & ~muted).sum() > 50 and (lv >= 0).sum() > (lv == 127).sum() > 0
        for s in (N.STATUS_DROP_AUTH, N.STATUS_SKIPPED, N.STATUS_DROP_INVALID):
            assert (st == s).sum() > 0, N.STATUS_NAMES[s]
        if mode == "array":
            assert (st == N.STATUS_DROP_REPLAY).sum() > 0
        # a muted packet ends authenticated, not deciphered; any other accepted one is the sender's plaintext
        for i in np.nonzero(ok)[0]:
            o, k = int(b.off[i]), int(ln[i])
            got = seg[o:o + k].tobytes()
            if muted[i] or b.flags[i] & DISCARD:
                assert got == b.protected[i][:k] if i not in b.replayed else True, i
            elif i not in b.replayed:
                assert got == b.plain[i], i
        assert any(muted[i] and ok[i] and b.protected[i][:int(ln[i])] != b.plain[i] for i in range(n))


@pytest.mark.parametrize("route", ["host", "device"])
def test_muted_among_tampered_and_replayed_against_the_oracle(eng, oracle, route):
    """Well-formed packets only, so that the oracle can run the existing call:
    muted packets (level 127) mixed with tampered tags and replays.  The oracle,
    given the reference's flags, authenticates the silent ones without
    deciphering them and drops what it dropped before; the _lvl call agrees with
    it to the byte."""
    keys = Keys(eng, CM, 7)
    b = Bundle(keys, 300, with_wild=False)
    ids = b.ids("array")
    want_lv, want_fl, _ = b.reference(ids)
    twin = Twin(eng)
    f = twin.factory(False, keys.mk, keys.ms, *keys.pols)
    t_ref, t_lvl = twin.transformer(O.KIND_RTP, f), twin.transformer(O.KIND_RTP, f)
    seg_w, ln_w, st_w = twin.run(t_ref, True, b.seg, b.off, b.len, b.cap, want_fl)  # oracle == engine, states too
    seg, ln, st, lv = run_lvl(eng, route, t_lvl.tid, b, ids, "array", b.flags)
    assert np.array_equal(lv, want_lv) and np.array_equal(st, st_w) and np.array_equal(ln, ln_w)
    assert np.array_equal(seg, seg_w)
    same_states(eng, [(t_lvl.e, t_ref.e)], b.ssrc)
    ok, muted = st == N.STATUS_OK, lv == 127
    assert (ok & muted).sum() > 10 and (st == N.STATUS_DROP_AUTH).sum() > 10 and (st == N.STATUS_DROP_REPLAY).sum() > 3
    assert ((st == N.STATUS_DROP_AUTH) & muted).sum() > 0  # a tampered muted packet is still dropped


def test_gcm_engine(eng_gcm):
    """One AES-GCM engine case (enable_aead): a silent packet's tag is checked and its payload left sealed."""
    keys = Keys(eng_gcm, GCM, 31)
    b = Bundle(keys, 300)
    st, lv, ln, seg = equivalent(keys, b, "device", "array")
    ok, muted = st == N.STATUS_OK, lv == 127
    assert (ok & muted).sum() > 5 and (ok & ~muted).sum() > 50 and (st == N.STATUS_DROP_AUTH).sum() > 0


@pytest.mark.parametrize("route", ["host", "device"])
def test_id_zero_is_the_plain_call(eng, route):
    """ext_id 0 and no ext_ids: byte for byte transform_device / transform_host with the caller's flags, and
    every level -128."""
    keys = Keys(eng, CM, 55)
    b = Bundle(keys, 300, wild_last=True)
    ra, rb = keys.receiver(), keys.receiver()
    s0 = eng.audio_level_stats()
    seg, ln, st, lv = run_lvl(eng, route, ra.tid, b, np.zeros(b.n, np.uint8), "scalar", b.flags)
    s1 = eng.audio_level_stats()
    seg_w, ln_w, st_w = run_plain(eng, route, rb.tid, b, b.flags)
    assert (lv == -128).all()
    assert np.array_equal(st, st_w) and np.array_equal(ln, ln_w) and np.array_equal(seg, seg_w)
    same_states(eng, [(ra, rb)], b.ssrc)
    assert (s1["calls"], s1["entries_read"], s1["levels_found"], s1["silent"]) == \
        (s0["calls"] + 1, s0["entries_read"], s0["levels_found"], s0["silent"])


def test_no_caller_flags(eng):
    """flags NULL: the engine's words are the stage's alone."""
    keys = Keys(eng, CM, 77)
    b = Bundle(keys, 64, wild_last=True)
    b.flags[:] = 0
    equivalent(keys, b, "device", "scalar", pass_flags=False)


def test_reverse_transform_levels(eng):
    """The Java-API mirror: FLAG_SILENCE set in pkt.flags, the dispatcher's tuples, dropped packets None."""
    keys = Keys(eng, CM, 91)
    b = Bundle(keys, 40, with_wild=False)
    rx = keys.receiver()
    want = [R.reverse_transform(p, len(p), len(p), 0, 1) for p in b.sent]
    late = [i for i in range(40) if want[i][0] >= 0 and i not in b.tampered][1]
    b.sent[late] = b.sent[late][:-1] + bytes([b.sent[late][-1] ^ 1])  # a packet with a level and a bad tag
    b.tampered.add(late)
    pkts = [RawPacket(bytearray(p)) for p in b.sent]
    out = reverse_transform_levels(pkts, rx, 1)
    assert len(out) == 40 and any(o is not None for o in out) and any(o is None for o in out)
    for i, (lv, fl) in enumerate(want):
        ssrc, ts = int.from_bytes(b.sent[i][8:12], "big"), int.from_bytes(b.sent[i][4:8], "big")
        assert out[i] == ((ssrc, 127 - lv, ts) if lv >= 0 else None), i
        if i in b.tampered:
            assert pkts[i] is None  # the level was reported all the same
        else:
            assert pkts[i].flags == fl
            assert pkts[i].data() == (b.protected[i][:pkts[i].length] if lv == 127 else b.plain[i]), i
    assert any(i in b.tampered and out[i] is not None for i in range(40))
