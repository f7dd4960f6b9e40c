"""The RFC 7714 AES-GCM profiles on the per-packet paths -- srtp_aggregator_submit
with callbacks, srtp_aggregator_transform, srtp_queue_submit / _reap,
srtp_rawpacket_transform / _transform_one and the JNI shim -- on an engine and
on a 2-shard dispatcher with the AES-GCM switch on.  GCM SRTCP appends 20
bytes, so these paths give protect srtp_engine_trailer_room() bytes of room: 20
when the aggregator or batch was created with the switch on, 16 otherwise.
Every packet is held to tests/gcm_ref.py, fed per transformer in the order the
path completed its packets."""
import ctypes as C
import threading

import numpy as np
import pytest

import gcm_ref as G
import test_gcm_engine as E
import test_jni_shim as S
from libjitsi_amd import RawPacket, SRTPAggregator, SRTPDispatcher, SRTPPolicy
from libjitsi_amd import _native as N

pytestmark = pytest.mark.gpu

RTP, RTCP = 0, 1
THREADS, PER = 4, 8  # per thread and stream: PER packets protected, then unprotected
DROPPED = "dropped"  # a path that only hands back None for a dropped packet


def make_target(engine_factory, which):
    if which == "engine":
        e = engine_factory(max_contexts=1 << 13, max_factories=128, max_transformers=512)
    else:
        e = SRTPDispatcher([0, 0], max_contexts=1 << 13, max_factories=128, max_transformers=512)
    e.enable_aead()
    return e


@pytest.fixture(scope="module", params=["engine", "dispatcher"])
def target(engine_factory, request):
    e = make_target(engine_factory, request.param)
    yield e
    if request.param == "dispatcher":
        e.close()


class Streams:
    """One thread's transformers: GCM-128 SRTP and SRTCP and an AES-CM SRTP
    stream, each as a sender / receiver pair, in the engine and in gcm_ref."""

    def __init__(self, eng, k):
        fg = E.F(eng, True, *E.keys(900 + k), E.GCM128)
        fa = E.F(eng, True, *E.keys(950 + k, 16, 14), *E.P80)
        self.pairs = [(E.T(RTP, fg), E.T(RTP, fg)), (E.T(RTCP, fg), E.T(RTCP, fg)), (E.T(RTP, fa), E.T(RTP, fa))]
        self.k = k

    def plain(self):
        """[(pair index, packet)]: PER + 1 packets per stream, interleaved."""
        out = []
        for i in range(PER + 1):
            out.append((0, G.rtp_packet(0x9000 + self.k, 50 + i, G.payload(5 + 61 * i, i), ext_words=i % 3 - 1)))
            out.append((1, G.rtcp_packet(0x9100 + self.k, G.payload(4 * (1 + 7 * i), i))))
            out.append((2, G.rtp_packet(0x9200 + self.k, 70 + i, G.payload(30 + i, i))))
        return out


def ref_one(tr, reverse, data, room):
    seg, off, ln, cap = G.pack([data], 0 if reverse else room)
    st = G.process(tr, reverse, seg, off, ln, cap)
    return int(st[0]), seg[:int(ln[0])].tobytes()


def check(jobs, results, room, order=None):
    """jobs[i] = (transformer T, reverse, data); results[i] = (status, bytes), or
    (DROPPED, None).  The reference takes the packets in `order` (the path's
    completion order; default: as submitted).  Returns the reference's statuses."""
    sts = [None] * len(jobs)
    for i in (order if order is not None else range(len(jobs))):
        t, reverse, data = jobs[i]
        st, out = ref_one(t.r, reverse, data, room)
        got_st, got = results[i]
        if got_st == DROPPED:
            assert st in (1, 2), (i, t.kind, reverse, st)
        else:
            assert got_st == st and got == out, (i, t.kind, reverse, got_st, st)
        sts[i] = st
    return sts


def two_phases(eng, path, room):
    """THREADS threads, each with its own streams: protect everything through
    `path`; then unprotect the results, with per stream one packet twice in a
    row (a replay) and its last packet only as a forgery (one flipped tag bit).
    path(jobs) -> (results, completion order or None)."""
    streams = [Streams(eng, k) for k in range(THREADS)]
    errs = []

    def work(k):
        try:
            s = streams[k]
            plain = s.plain()
            jobs = [(s.pairs[p][0], False, d) for p, d in plain]
            res, order = path(jobs)
            assert check(jobs, res, room, order) == [0] * len(jobs)
            sealed = [(p, r[1]) for (p, _), r in zip(plain, res)]
            jobs2 = []
            for i, (p, d) in enumerate(sealed):
                if i >= 3 * PER:  # the stream's last packet: forged
                    bad = bytearray(d)
                    bad[-6 if p == 1 else -2] ^= 0x20  # in the tag (SRTCP: before the E|index word)
                    d = bytes(bad)
                jobs2.append((s.pairs[p][1], True, d))
                if i in (9, 10, 11):  # the same packet again: a replay
                    jobs2.append((s.pairs[p][1], True, d))
            res2, order2 = path(jobs2)
            sts = check(jobs2, res2, room, order2)
            assert sts.count(1) == 3 and sts.count(2) == 3 and sts.count(0) == 3 * PER, sts
            for (t, _, _), (st, out), (p, d) in zip(jobs2[:9], res2[:9], plain[:9]):
                assert st == 0 and out == d  # round trip
        except BaseException as ex:  # noqa: BLE001 -- raised again by the main thread
            errs.append(ex)

    th = [threading.Thread(target=work, args=(k,)) for k in range(THREADS)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]


def small_agg(target, cb=None):
    return SRTPAggregator(target, cb, max_packets=256, max_bytes=1 << 20, deadline_us=200)


def test_trailer_room(target):
    agg = small_agg(target)
    try:
        assert agg.trailer_room == 20
        if not isinstance(target, SRTPDispatcher):
            assert target.trailer_room == 20
    finally:
        agg.close()


def test_aggregator_submit_callbacks(target):
    done, seq, lock, nxt = {}, [], threading.Condition(), [0]

    def cb(cookie, status, data):
        with lock:
            done[cookie] = (status, data)
            seq.append(cookie)
            lock.notify_all()

    agg = small_agg(target, cb)

    def path(jobs):
        with lock:
            base = nxt[0]
            nxt[0] += len(jobs)
        for i, (t, reverse, data) in enumerate(jobs):
            assert agg.submit(reverse, t.e, data, cookie=base + i) == 0
        agg.flush()  # seals now; it counts every thread's packets, so it is no barrier for this thread's
        with lock:
            assert lock.wait_for(lambda: all(base + i in done for i in range(len(jobs))), timeout=60)
            order = [c - base for c in seq if base <= c < base + len(jobs)]
            res = [done[base + i] for i in range(len(jobs))]
        assert sorted(order) == list(range(len(jobs)))
        return res, order

    try:
        two_phases(target, path, agg.trailer_room)
    finally:
        agg.close()


def test_aggregator_transform(target):
    agg = small_agg(target)
    try:
        two_phases(target, lambda jobs: ([agg.transform(r, t.e, d) for t, r, d in jobs], None), agg.trailer_room)
    finally:
        agg.close()


def test_queue(target):
    L = N.lib()
    agg = small_agg(target)
    room = agg.trailer_room

    def path(jobs):
        q = C.c_void_p()
        assert L.srtp_queue_create(agg.h, 64, C.byref(q)) == 0
        try:
            res, order = [None] * len(jobs), []
            comps = (N.Completion * 64)()

            def reap():
                k = L.srtp_queue_reap(q, comps, 64, 1)
                assert k >= 0
                for c in comps[:k]:
                    res[c.cookie] = (c.status, C.string_at(c.data, c.len) if c.len else b"")
                    order.append(int(c.cookie))
                L.srtp_queue_release(q)

            for i, (t, reverse, data) in enumerate(jobs):
                cap = len(data) if reverse else len(data) + room
                while True:
                    rc = L.srtp_queue_submit(q, int(reverse), t.tid, data, len(data), len(data), cap, 0, i)
                    if rc != N.EAGAIN:
                        break
                    reap()
                assert rc == 0
            while len(order) < len(jobs):
                reap()
            return res, order
        finally:
            L.srtp_queue_destroy(q)

    try:
        two_phases(target, path, room)
    finally:
        agg.close()


def _result(p):
    return (0, p.data()) if p is not None else (DROPPED, None)


def test_rawpacket_transform_one(target):
    """SRTPTransformer.transform(RawPacket): srtp_rawpacket_transform_one."""
    def path(jobs):
        return [_result(t.e.reverseTransform(RawPacket(bytearray(d))) if r else t.e.transform(RawPacket(bytearray(d))))
                for t, r, d in jobs], None

    two_phases(target, path, 20)


def test_rawpacket_transform_array(target):
    """transform(RawPacket[]): srtp_rawpacket_transform, an array per transformer."""
    def path(jobs):
        res, by_t = [None] * len(jobs), {}
        for i, (t, reverse, _) in enumerate(jobs):
            by_t.setdefault(id(t), (t, reverse, []))[2].append(i)
        for t, reverse, idx in by_t.values():
            pk = [RawPacket(bytearray(jobs[i][2])) for i in idx]
            out = t.e.reverseTransform(pk) if reverse else t.e.transform(pk)
            for i, p in zip(idx, out):
                res[i] = _result(p)
        return res, [i for _, _, idx in by_t.values() for i in idx]

    two_phases(target, path, 20)


# ------------------------------------------------------- RawPacket write-back
@pytest.mark.parametrize("kind,extra", [(RTCP, 20), (RTCP, 19), (RTCP, 0), (RTP, 16), (RTP, 15), (RTP, 0)])
def test_write_back(target, kind, extra):
    """A buffer with exactly `extra` bytes behind the packet, the packet at an
    offset.  SRTCP protect is RawPacket.grow: always a new buffer of exactly
    the new length at offset 0.  SRTP protect is RawPacket.append: in place
    with room for the 16-byte tag, else a new buffer of exactly length + 16."""
    snd, rcv = E.sender_receiver(target, kind, E.GCM128, 980 + 32 * kind + extra)
    grow = 20 if kind == RTCP else 16

    def pkt(i):
        return G.rtcp_packet(0x9400, G.payload(40, i)) if kind == RTCP else G.rtp_packet(0x9401, 7 + i, G.payload(40, i))

    for as_array in (False, True):  # srtp_rawpacket_transform_one, srtp_rawpacket_transform
        data, data2 = pkt(2 * as_array), pkt(2 * as_array + 1)
        p, q = RawPacket(b"\xee" * 5 + data + b"\xdd" * extra, 5, len(data)), RawPacket(data2)
        buf = p.buffer  # (RawPacket copies what it is given)
        if as_array:
            out = snd.e.transform([p, q])
            assert out[0] is p and out[1] is q
        else:
            assert snd.e.transform(p) is p
        assert (0, p.data()) == ref_one(snd.r, False, data, 20) and p.length == len(data) + grow
        if as_array:
            assert (0, q.data()) == ref_one(snd.r, False, data2, 20)
        if kind == RTP and extra >= 16:
            assert p.buffer is buf and p.offset == 5 and bytes(buf[:5]) == b"\xee" * 5
            assert bytes(buf[5 + p.length:]) == b"\xdd" * (extra - 16)
        else:
            assert p.buffer is not buf and p.offset == 0 and len(p.buffer) == p.length
        back = rcv.e.reverseTransform(RawPacket(bytearray(p.data())))
        assert back is not None and back.data() == data


# -------------------------------------------------------------- compatibility
def test_created_before_the_switch(engine_factory):
    """An engine without the switch reports 16; an aggregator created before the
    switch is turned on keeps 16, and GCM SRTCP protect through it still answers
    ERR_CAPACITY (GCM SRTP fits); one created afterwards has 20."""
    e = engine_factory(max_contexts=1024, max_factories=8, max_transformers=8)
    assert e.trailer_room == 16 and N.lib().srtp_trailer_room(0) == 16
    early = small_agg(e)
    e.enable_aead()
    late = small_agg(e)
    try:
        assert early.trailer_room == 16 and late.trailer_room == 20 and e.trailer_room == 20
        f = E.F(e, True, *E.keys(990), E.GCM128)
        c, r = E.T(RTCP, f), E.T(RTP, f)
        pc, pr = G.rtcp_packet(0x9500, G.payload(24, 1)), G.rtp_packet(0x9501, 3, G.payload(24, 2))
        st, out = early.transform(False, c.e, pc)
        assert st == N.STATUS_ERR_CAPACITY and out == pc
        assert early.transform(False, r.e, pr) == ref_one(r.r, False, pr, 16)
        assert late.transform(False, c.e, pc) == ref_one(c.r, False, pc, 20)
        e.enable_aead(False)
        assert e.trailer_room == 16 and late.trailer_room == 20
    finally:
        early.close()
        late.close()


# ------------------------------------------------------------------- the shim
class GcmJvm(S.Jvm):
    """S.Jvm with SrtpMi355x.dispatch()'s AEAD step: dispatchEnableAead right
    after dispatchCreate, before aggregatorCreate."""

    def __init__(self, n_shards=2):
        self.L, self.J = S.load()
        self.env, self.cls = self.L.fj_env(), self.L.fj_rawpacket_class()
        devs = np.zeros(n_shards, np.int32)
        self.d = self.J("dispatchCreate")(self.env, self.cls, self.L.fj_new_ints(devs.ctypes.data, n_shards),
                                          1, 1 << 14)
        assert self.d
        en = self.J("dispatchEnableAead")
        en.argtypes, en.restype = [S.vp, S.vp, S.i64, S.u8], S.i32
        assert en(self.env, self.cls, self.d, 1) == 0
        self.agg = self.J("aggregatorCreate")(self.env, self.cls, self.d, 0, 0, 0)
        assert self.agg


def test_shim_exports_every_java_native():
    L, J = S.load()
    names = S.java_natives()
    assert "dispatchEnableAead" in names
    for n in names:
        J(n)


def test_shim_gcm():
    """transformOne and transformPackets for GCM SRTP and SRTCP through the JNI
    shim, as GpuTransformerBase calls them, against gcm_ref."""
    jvm = GcmJvm()
    try:
        mk, ms = E.keys(995)
        pol = SRTPPolicy(*E.GCM128)
        f = jvm.factory(True, mk, ms, pol)
        rf = G.Factory(True, mk, ms, E.GCM128, E.GCM128)
        for kind in (RTP, RTCP):
            ts, tr = jvm.transformer(kind, f, f), jvm.transformer(kind, f, f)
            rs, rr = G.Transformer(kind, rf, rf), G.Transformer(kind, rf, rf)
            mk_pkt = (lambda i: G.rtp_packet(0x9600, 20 + i, G.payload(33 + 50 * i, i))) if kind == RTP else \
                (lambda i: G.rtcp_packet(0x9601, G.payload(12 + 16 * i, i)))
            sealed = []
            for i in range(3):  # per packet; with room behind the packet only SRTP stays in place
                data = mk_pkt(i)
                extra = 24 if i == 1 else 0
                p = jvm.packet(data, 3 if extra else 0, extra)
                b0 = jvm.L.fj_packet_buffer(p)
                assert jvm.one(False, ts, p) == 0
                got, b = jvm.packet_bytes(p)
                assert (0, got) == ref_one(rs, False, data, 20)
                assert (b == b0) == (kind == RTP and extra > 0)
                sealed.append(got)
            plain = [mk_pkt(i) for i in range(3, 8)]
            r, out = jvm.array(False, ts, [jvm.packet(x) for x in plain])  # the array path
            assert r == 0
            for x, p in zip(plain, out):
                got, _ = jvm.packet_bytes(p)
                assert (0, got) == ref_one(rs, False, x, 20)
                sealed.append(got)
            bad = bytearray(sealed[6])
            bad[-7] ^= 4
            inputs = sealed[:6] + [bytes(bad), sealed[5], sealed[7]]  # a forgery, then the last accepted one again
            r, out = jvm.array(True, tr, [jvm.packet(x) for x in inputs])
            assert r == 0
            for i, (x, p) in enumerate(zip(inputs, out)):
                st, want = ref_one(rr, True, x, 0)
                assert st == (2 if i == 6 else 1 if i == 7 else 0)
                assert (p is None or not p) == (st != 0)
                if st == 0:
                    assert jvm.packet_bytes(p)[0] == want
            p = jvm.packet(sealed[6])
            assert jvm.one(True, tr, p) == 0 and jvm.packet_bytes(p)[0] == ref_one(rr, True, sealed[6], 0)[1]
    finally:
        jvm.close()
