"""Small bundles of an engine that holds AES-GCM key sets in one launch: k_small's
GCM instance (srtp_stats.small_aead_bundles).  Which bundles take it; its
results against tests/gcm_ref.py on test_gcm_engine.py's cases, each wrapped so
that it also shows the route it ran on; against the multi-kernel chain
(SRTP_DEBUG_NO_SMALL) bit for bit on bundles that mix GCM and AES-CM + HMAC key
sets, at the sizes where the kernel's shape changes (one packet, fewer packets
than waves, a full workgroup, the hand-off to a second workgroup, a wave with
two packets, the limit); one stream whose ROC rolls over inside the walk's GCM
chain; the lone packet; and the per-packet paths (direct mode).

The route is limited to srtp_small_aead_max() packets (kSmallGcmMax = 8, one
packet per wave of the workgroup that verifies the tags before the walk): in
the sweep of profiles/gcm_small/ the one-launch route loses to the chain from
16 packets on.  SRTP_DEBUG_FORCE_SMALL lifts the limit to
k_small's own 255 packets; the parity cases run with it, so that they reach the
instance at every size, its several workgroups included, and the route test
and the lone-packet and per-packet tests run without it."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import gcm_ref as G
import test_gcm_engine as E
import test_gcm_per_packet as P
import test_gcm_wave_engine as W
from harness import Twin
from libjitsi_amd import SRTPAggregator, profile_policies, synth
from libjitsi_amd import _native as N

pytestmark = pytest.mark.gpu

RTP, RTCP = E.RTP, E.RTCP
SMALL_MAX = 255  # srtp_kernels.h kSmallMaxN
OFF_FLAGS = ("DEBUG_NO_SMALL", "DEBUG_NO_GCM_WAVE", "DEBUG_FORCE_GCM_WAVE", "DEBUG_NO_WIDE", "DEBUG_FORCE_WIDE",
             "DEBUG_FORCE_CHAIN_STALL")


def counts(e):
    s = e.stats()
    return np.array([s["small_aead_bundles"], s["small_bundles"], s["bundles"]], np.int64)


@contextmanager
def on_the_route(e):
    """The body's bundles ran on the GCM instance: its counter advanced, and by
    as much as the engine's bundle count; k_small's other counter stood still."""
    c0 = counts(e)
    yield
    d = counts(e) - c0
    assert d[0] > 0 and d[1] == 0 and d[0] == d[2], d.tolist()


@pytest.fixture(scope="module")
def eng(engine_factory):
    return W.make(engine_factory, N.DEBUG_FORCE_SMALL)


@pytest.fixture(scope="module")
def eng_noabort(engine_factory):
    return W.make(engine_factory, N.DEBUG_FORCE_SMALL, abort_on_error=False)


@pytest.fixture(scope="module")
def eng_default(engine_factory):
    return E.make_engine(engine_factory)


# ------------------------------------------------------------------ 1. routes
def _round_trip(e, snd, rcv, n, ssrc0, seq0):
    """n short packets protected and unprotected (each held to gcm_ref);
    returns the counters' movement per direction."""
    n_ssrc = max(1, n // 25)
    pk = [G.rtp_packet(ssrc0 + i % n_ssrc, seq0 + i // n_ssrc, G.payload(16, i)) for i in range(n)]
    seg, off, ln, cap = E.pack(pk, room=16)
    c0 = counts(e)
    seg2, ln2, st = E.run(e, snd, False, seg, off, ln, cap)
    c1 = counts(e)
    _, ln3, st3 = E.run(e, rcv, True, seg2, off, ln2, cap)
    c2 = counts(e)
    assert st.tolist() == [0] * n and st3.tolist() == [0] * n and np.array_equal(ln3, ln)
    return (c1 - c0)[:2].tolist(), (c2 - c1)[:2].tolist()


def test_routes(engine_factory):
    """Which bundles take the GCM instance.  Its limit is srtp_small_aead_max()
    = 8 packets, not k_small's 255: in profiles/gcm_small/sweep.json the
    one-launch route's median lies below the chain's by more than the chain's
    p90 - p10 at 1, 4 and 8 packets in both directions, and no longer at 16 (GCM
    unprotect 79.4 us on the chain, 83.6 us in one launch; 81 against 223 us at
    64).  So GCM bundles of 1 and 8 packets each add 1 to small_aead_bundles
    and 0 to small_bundles, in both directions; 9, 16, 17, 255 and 256 add to
    neither; with SRTP_DEBUG_FORCE_SMALL the limit is 255.  The same holds for
    the engine's AES-CM + HMAC bundles (1 and 40 packets)."""
    e = E.make_engine(engine_factory)
    fg, fa = E.F(e, True, *E.keys(800), E.GCM128), E.F(e, True, *E.keys(801, 16, 14), *E.P80)
    gs, gr, as_, ar = E.T(RTP, fg), E.T(RTP, fg), E.T(RTP, fa), E.T(RTP, fa)
    cap = int(N.lib().srtp_small_aead_max())
    assert cap == 8
    seq = 1
    # GCM bundles, and AES-CM + HMAC bundles of the same engine: the GCM instance,
    # both directions, up to its limit; with FORCE_SMALL up to k_small's
    for force in (False, True):
        e.set_debug(N.DEBUG_FORCE_SMALL if force else 0)
        for n in (1, cap, cap + 1, 16, 17, SMALL_MAX, SMALL_MAX + 1):
            took = [1, 0] if n <= (SMALL_MAX if force else cap) else [0, 0]
            assert _round_trip(e, gs, gr, n, 0x80000, seq) == (took, took), (force, n)
            seq += 30
        for n in (1, 40):
            took = [1, 0] if n <= (SMALL_MAX if force else cap) else [0, 0]
            assert _round_trip(e, as_, ar, n, 0x81000, seq) == (took, took), (force, n)
            seq += 30
    e.set_debug(0)
    for name in OFF_FLAGS:  # every hook that needs the chain keeps a bundle off the route
        for flags in (getattr(N, name), getattr(N, name) | N.DEBUG_FORCE_SMALL):
            e.set_debug(flags)
            try:
                assert _round_trip(e, gs, gr, 5, 0x80000, seq) == ([0, 0], [0, 0]), name
            finally:
                e.set_debug(0)
            seq += 30
    # the switch on and no GCM factory: the instances of always
    e2 = E.make_engine(engine_factory)
    f2 = E.F(e2, True, *E.keys(802, 16, 14), *E.P80)
    assert _round_trip(e2, E.T(RTP, f2), E.T(RTP, f2), 7, 0x82000, 1) == ([0, 1], [0, 1])
    # a key set that is neither the split path's nor GCM: the chain for every bundle
    for k, name in enumerate(("F8_128_HMAC_SHA1_80", "AES_CM_128_SKEIN_32")):
        e3 = E.make_engine(engine_factory)
        f3 = E.F(e3, True, *E.keys(803 + k), E.GCM128)
        sp, cp = (E.tup(p) for p in profile_policies(name))
        E.F(e3, True, *E.keys(805 + k, 16, 14), sp, cp)
        assert _round_trip(e3, E.T(RTP, f3), E.T(RTP, f3), 5, 0x83000, 1) == ([0, 0], [0, 0]), name


# ------------------------------------------- 2. parity with the reference
def test_golden(eng):
    with on_the_route(eng):
        E.test_golden(eng)


@pytest.mark.parametrize("pol", [E.GCM128, E.GCM256], ids=["128", "256"])
def test_lengths(eng, pol):
    with on_the_route(eng):
        E.test_lengths(eng, pol)


@pytest.mark.parametrize("abort", [False, True], ids=["each", "abort"])
def test_reject_shapes(eng, eng_noabort, abort):
    """Among them the single 8-byte SRTCP packet and the capacities around 16 and 20."""
    with on_the_route(eng if abort else eng_noabort):
        E.test_reject_shapes(eng, eng_noabort, abort)


def test_tampering(eng):
    with on_the_route(eng):
        E.test_tampering(eng)


def test_state(eng):
    """Among it DISCARD / SILENCE, and a ROC the walk overturns: gcm_reverify
    reads the S that this route's verify pass wrote."""
    with on_the_route(eng):
        E.test_state(eng)


def test_srtcp_e0(eng):
    with on_the_route(eng):
        E.test_srtcp_e0(eng)


def test_mixed_engine(engine_factory):
    """E.test_mixed_engine creates an F8 and a Skein factory before its first
    bundle, and an engine that holds either keeps every bundle on the chain
    (test_routes): so the case runs on an engine of its own and must move
    neither counter.  What it is about -- 70 GCM key sets in one bundle beside
    AES-CM + HMAC ones, factories with a GCM policy on one side only -- runs
    on the route in test_mixed_key_sets."""
    e = E.make_engine(engine_factory)
    c0 = counts(e)
    E.test_mixed_engine(e)
    assert (counts(e) - c0)[:2].tolist() == [0, 0]


def test_mixed_key_sets(eng):
    """E.test_mixed_engine without its F8 and Skein factories."""
    pairs = [E.sender_receiver(eng, RTP, E.GCM128 if i % 2 else E.GCM256, 1100 + i) for i in range(70)]
    f = E.F(eng, True, *E.keys(1180, 16, 14), *E.P80)
    pairs.append((E.T(RTP, f), E.T(RTP, f)))
    fm = E.F(eng, True, *E.keys(1190, 16, 14), E.GCM128, E.P80[1])  # GCM SRTP, HMAC SRTCP
    fm2 = E.F(eng, True, *E.keys(1191, 16, 14), E.P80[0], E.GCM128)  # and the other way round
    pairs += [(E.T(RTP, fm), E.T(RTP, fm)), (E.T(RTP, fm2), E.T(RTP, fm2))]
    cms = [(E.T(RTCP, fm), E.T(RTCP, fm)), (E.T(RTCP, fm2), E.T(RTCP, fm2))]
    items = []
    for rnd in range(2):
        for k, (s, r) in enumerate(pairs):
            items.append((s, r, G.rtp_packet(0xD000 + k, 20 + rnd, G.payload(16 + (k % 5), k + rnd))))
        for k, (s, r) in enumerate(cms):
            items.append((s, r, G.rtcp_packet(0xD800 + k, G.payload(16, k + rnd))))
    seg, off, ln, cap = E.pack([p for _, _, p in items], room=24)
    with on_the_route(eng):
        seg2, ln2, st = E.run(eng, [s for s, _, _ in items], False, seg, off, ln, cap)
        seg3, ln3, st3 = E.run(eng, [r for _, r, _ in items], True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * len(items) and st3.tolist() == [0] * len(items) and np.array_equal(ln3, ln)
    for i in range(len(items)):
        assert seg3[off[i]:off[i] + ln[i]].tobytes() == items[i][2]


# ------------------------------------- 3. parity with the chain, bit for bit
@pytest.mark.parametrize("n", [1, 4, 5, 16, 17, 33, SMALL_MAX])
def test_mixed_bundle_against_the_chain(engine_factory, n):
    """test_gcm_wave_engine's mixed bundle on the one-launch route (a default
    engine up to srtp_small_aead_max() packets; FORCE_SMALL, which changes
    nothing there, for the larger ones) and on a NO_SMALL twin, protect then unprotect: each against gcm_ref (E.run), and the two
    bit-equal in status, length, the segment with the room behind each packet
    and every exported context."""
    outs = []
    for flags in (N.DEBUG_FORCE_SMALL, N.DEBUG_NO_SMALL):
        e = W.make(engine_factory, flags)
        items, pf = W._mixed(e, n)
        seg, off, ln, cap = E.pack([p for _, _, p in items], room=24)
        c0 = counts(e)
        seg2, ln2, st = E.run(e, [s for s, _, _ in items], False, seg, off, ln, cap, flags=pf)
        seg3, ln3, st3 = E.run(e, [r for _, r, _ in items], True, seg2, off, ln2, cap, flags=pf)
        assert (counts(e) - c0)[:2].tolist() == ([2, 0] if flags == N.DEBUG_FORCE_SMALL else [0, 0])
        want = [9 if f else 0 for f in pf]
        assert st.tolist() == want and st3.tolist() == want
        for i, (_, _, p) in enumerate(items):
            assert seg3[off[i]:off[i] + ln3[i]].tobytes() == p
        ex = []
        for t in sorted({id(t): t for s, r, _ in items for t in (s, r)}.values(), key=lambda t: t.tid):
            ex.append(sorted((ssrc, sorted(stt.items())) for ssrc, stt in e.export_contexts(t.e).items()))
        outs.append((st.tolist(), ln2.tolist(), seg2.tobytes(), st3.tolist(), ln3.tolist(), seg3.tobytes(), ex))
    assert outs[0] == outs[1]


# ------------------------------------------------- 4. one stream, one chain
@pytest.mark.parametrize("kind,n,first", [(RTP, SMALL_MAX, 65400), (RTP, 40, 65535), (RTCP, 60, 0)],
                         ids=["rtp255_from_65400", "rtp40_from_65535", "rtcp60"])
def test_one_stream(eng, kind, n, first):
    """Every packet of the bundle on one SSRC: one walk_one_gcm chain through
    the tile, the ROC rolling over inside it; state included (E.run)."""
    snd, rcv = E.sender_receiver(eng, kind, E.GCM128, 1200 + n)
    if kind == RTP:
        pk = E._stream(0xF1000 + n, range(first, first + n))
    else:
        pk = [G.rtcp_packet(0xF2000, G.payload(12 + 4 * (i % 5), i)) for i in range(n)]
    seg, off, ln, cap = E.pack(pk, room=24)
    with on_the_route(eng):
        seg2, ln2, st = E.run(eng, snd, False, seg, off, ln, cap)
        seg3, ln3, st3 = E.run(eng, rcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * n and st3.tolist() == [0] * n and np.array_equal(ln3, ln)
    for i, p in enumerate(pk):
        assert seg3[off[i]:off[i] + ln3[i]].tobytes() == p
    if kind == RTP:
        assert eng.context_state(rcv.e, 0xF1000 + n)["roc"] == 1


# ------------------------------------------------------- 5. the lone packet
LONE = [(RTP, 0), (RTP, 1), (RTP, 16), (RTP, 1188), (RTCP, 0), (RTCP, 192)]


@pytest.mark.parametrize("kind,body", LONE, ids=["%s_%d" % ("rtcp" if k else "rtp", b) for k, b in LONE])
def test_lone_gcm_packet(eng_default, kind, body):
    """n = 1, both directions, no debug flag: the image is filled before the
    verify pass and the wave MAC is skipped.  The 8-byte SRTCP packet is refused
    as the reference refuses it (the shape that faulted an earlier build of the
    chain)."""
    eng = eng_default
    snd, rcv = E.sender_receiver(eng, kind, E.GCM128, 1300 + body + kind)
    p = G.rtp_packet(0xF3000 + body, 9, G.payload(body, body)) if kind == RTP else G.rtcp_packet(0xF4000 + body, G.payload(body, body))
    assert len(p) == (12 if kind == RTP else 8) + body
    seg, off, ln, cap = E.pack([p], room=24)
    with on_the_route(eng):
        seg2, ln2, st = E.run(eng, snd, False, seg, off, ln, cap)
        seg3, ln3, st3 = E.run(eng, rcv, True, seg2, off, ln2, cap)
    if len(p) >= 12:
        assert st.tolist() == [0] and st3.tolist() == [0] and seg3[:int(ln3[0])].tobytes() == p
    else:
        assert st.tolist() == [7] and st3.tolist() == [7]


@pytest.mark.parametrize("plen", [0, 50, 1188])
def test_lone_aes_cm_packet(eng_default, oracle, plen):
    """A lone AES-CM + HMAC packet on the engine that holds GCM key sets: the
    GCM instance keeps the wave MAC and the late fill of the image for it.
    Held to the oracle, as test_k_small.py holds k_small."""
    eng = eng_default
    from oracle import oracle as O
    E.F(eng, True, *E.keys(1399), E.GCM128)  # the engine holds a GCM key set, whichever test ran first
    twin = Twin(eng)
    (k, s), = synth.keys(1400 + plen, 1)
    pols = profile_policies("AES_CM_128_HMAC_SHA1_80")
    f = twin.factory(True, k, s, *pols)
    snd, rcv = twin.transformer(O.KIND_RTP, f), twin.transformer(O.KIND_RTP, f)
    p = G.rtp_packet(0xF5000 + plen, 77, G.payload(plen, plen))
    seg, off, ln, cap = E.pack([p], room=24)
    with on_the_route(eng):
        seg2, ln2, st = twin.run(snd, False, seg, off, ln, cap)
        seg3, ln3, st3 = twin.run(rcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] and st3.tolist() == [0] and np.asarray(seg3)[:int(ln3[0])].tobytes() == p


# ---------------------------------------------------- 6. the per-packet paths
def test_per_packet_paths(engine_factory):
    """srtp_aggregator_transform with a lone GCM SRTCP, GCM SRTP and AES-CM
    packet, each protected and unprotected, and a queue burst of 64 mixed
    packets, on an aggregator created after the switch: every bundle of theirs
    is one launch of the GCM instance (direct mode for the lone calls)."""
    e = P.make_target(engine_factory, "engine")
    s = P.Streams(e, 40)
    agg = SRTPAggregator(e, None, max_packets=256, max_bytes=1 << 20, deadline_us=200)
    L = N.lib()
    try:
        room = agg.trailer_room
        assert room == 20
        lone = [(1, G.rtcp_packet(0x9100 + s.k, G.payload(40, 1))), (0, G.rtp_packet(0x9000 + s.k, 50, G.payload(300, 2))),
                (2, G.rtp_packet(0x9200 + s.k, 70, G.payload(300, 3)))]
        with on_the_route(e):
            for p, d in lone:
                jobs = [(s.pairs[p][0], False, d)]
                res = [agg.transform(False, jobs[0][0].e, d)]
                assert P.check(jobs, res, room) == [0]
                jobs = [(s.pairs[p][1], True, res[0][1])]
                res = [agg.transform(True, jobs[0][0].e, jobs[0][2])]
                assert P.check(jobs, res, room) == [0] and res[0][1] == d

        def burst(jobs):
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

        plain = []
        for i in range(64):
            p = i % 3
            if p == 1:
                plain.append((p, G.rtcp_packet(0x9100 + s.k, G.payload(8 + 4 * (i % 7), i))))
            else:
                plain.append((p, G.rtp_packet(0x9000 + 0x200 * (p // 2) + s.k, 100 + i, G.payload(20 + i, i))))
        e.set_debug(N.DEBUG_FORCE_SMALL)  # a burst's bundles may hold more than srtp_small_aead_max() packets
        with on_the_route(e):
            jobs = [(s.pairs[p][0], False, d) for p, d in plain]
            res, order = burst(jobs)
            assert P.check(jobs, res, room, order) == [0] * 64
            jobs2 = [(s.pairs[p][1], True, r[1]) for (p, _), r in zip(plain, res)]
            res2, order2 = burst(jobs2)
            assert P.check(jobs2, res2, room, order2) == [0] * 64
            assert [r[1] for r in res2] == [d for _, d in plain]
    finally:
        agg.close()
