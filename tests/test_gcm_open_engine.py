"""The one-pass GCM open (k_gcm<open> / <fix>, k_gcm_wave<open> / <fix>): the
pass before the walk checks a packet's tag and deciphers it in the same trip,
the pass after the walk repairs the packets whose verdict the walk overturned.
A route is the lane or the wave kernels crossed with one pass or two
(SRTP_DEBUG_FORCE_GCM_SPEC / _NO_GCM_SPEC: the lane kernels' one-pass modes are
no size's default, profiles/gcm_open); results must not differ by a bit between them, nor
from tests/gcm_ref.py.  The cases are test_gcm_engine.py's on the four routes,
test_gcm_wave_engine's mixed bundles one-pass against two-pass, one bundle of
every way a verdict is overturned with the srtp_gcm_stats counts it implies,
the default route on both sides of launch_gcm's size rule, and the paths that
must not notice: k_small, protect, engines without GCM key sets, a dispatcher's
summed counters."""
import ctypes as C

import numpy as np
import pytest

import gcm_ref as G
import test_gcm_engine as E
import test_gcm_wave_engine as W
from libjitsi_amd import SRTPDispatcher
from libjitsi_amd import _native as N
from oracle import pyref

pytestmark = pytest.mark.gpu

RTP, RTCP = E.RTP, E.RTCP
ROUTES = {
    "lane_fused": N.DEBUG_NO_GCM_WAVE | N.DEBUG_FORCE_GCM_SPEC,
    "lane_two_pass": N.DEBUG_NO_GCM_WAVE | N.DEBUG_NO_GCM_SPEC,
    "wave_fused": N.DEBUG_FORCE_GCM_WAVE | N.DEBUG_FORCE_GCM_SPEC,
    "wave_two_pass": N.DEBUG_FORCE_GCM_WAVE | N.DEBUG_NO_GCM_SPEC,
}
ZERO = {"opened": 0, "restored": 0, "late": 0}


def make(engine_factory, flags, **kw):
    """An engine that keeps `flags` whatever a case sets on top (test_chains
    sets and clears FORCE_CHAIN_STALL): SRTPEngine.set_debug ORs them in."""
    e = E.make_engine(engine_factory, **kw)
    e._env_debug |= flags
    e.set_debug(0)
    return e


@pytest.fixture(scope="module", params=list(ROUTES), ids=list(ROUTES))
def route(request):
    return request.param


@pytest.fixture(scope="module")
def eng(engine_factory, route):
    return make(engine_factory, ROUTES[route])


@pytest.fixture(scope="module")
def eng_noabort(engine_factory, route):
    return make(engine_factory, ROUTES[route], abort_on_error=False)


def delta(e, before):
    now = e.gcm_stats()
    return {k: now[k] - before[k] for k in now}


# ------------------------------------------- 1. the existing cases, four routes
def test_golden(eng):
    E.test_golden(eng)


@pytest.mark.parametrize("pol", [E.GCM128, E.GCM256], ids=["128", "256"])
def test_lengths(eng, pol):
    E.test_lengths(eng, pol)


@pytest.mark.parametrize("abort", [False, True], ids=["each", "abort"])
def test_reject_shapes(eng, eng_noabort, abort):
    E.test_reject_shapes(eng, eng_noabort, abort)


def test_tampering(eng, route):
    g0 = eng.gcm_stats()
    E.test_tampering(eng)
    d = delta(eng, g0)
    # a forged packet is put back before the open pass ends: never counted as restored
    assert d["restored"] == 0 and (d["opened"] > 0) == route.endswith("fused")


def test_state(eng, route):
    g0 = eng.gcm_stats()
    E.test_state(eng)
    d = delta(eng, g0)
    if route.endswith("fused"):  # duplicates were restored, overturned ROC guesses deciphered late
        assert d["opened"] > 0 and d["restored"] > 0 and d["late"] > 0
    else:
        assert d == ZERO


def test_srtcp_e0(eng):
    g0 = eng.gcm_stats()
    E.test_srtcp_e0(eng)
    assert delta(eng, g0) == ZERO  # E = 0: nothing to decipher on any route


@pytest.mark.parametrize("stall", [False, True], ids=["plain", "forced_stall"])
def test_chains(eng, stall):
    E.test_chains(eng, stall)


# ------------------------------------------ 2. mixed bundles, one pass against two
def _mixed_run(e, n):
    items, flags = W._mixed(e, n)
    s0 = e.stats()
    seg, off, ln, cap = E.pack([p for _, _, p in items], room=24)
    seg2, ln2, st = E.run(e, [s for s, _, _ in items], False, seg, off, ln, cap, flags=flags)
    seg3, ln3, st3 = E.run(e, [r for _, r, _ in items], True, seg2, off, ln2, cap, flags=flags)
    want = [9 if f else 0 for f in flags]
    assert st.tolist() == want and st3.tolist() == want
    for i, (_, _, p) in enumerate(items):
        assert seg3[off[i]:off[i] + ln3[i]].tobytes() == p
    ex = []
    for t in sorted({id(t): t for s, r, _ in items for t in (s, r)}.values(), key=lambda t: t.tid):
        ex.append(sorted((ssrc, sorted(stt.items())) for ssrc, stt in e.export_contexts(t.e).items()))
    s1 = e.stats()
    # GCM packets with data: each is deciphered once, by the open pass or after the walk
    n_data = sum(1 for i, (s, _, p) in enumerate(items)
                 if not flags[i] and (s.r.fwd.srtcp if s.kind == RTCP else s.r.fwd.srtp)[0] == G.GCM
                 and len(p) > (8 if s.kind == RTCP else pyref.header_len(bytearray(p), len(p))))
    return (st.tolist(), ln2.tolist(), seg2.tobytes(), st3.tolist(), ln3.tolist(), seg3.tobytes(), ex,
            s1["roc_rechecks"] - s0["roc_rechecks"], s1["repaired"] - s0["repaired"]), n_data


@pytest.mark.parametrize("n", [1, 4, 5, 65, 300])
@pytest.mark.parametrize("kernels", ["lane", "wave"])
def test_mixed_bundle_fused_against_two_pass(engine_factory, kernels, n):
    """One wave, one workgroup of the wave kernel, its edge, a second wave of
    the lane kernel, several workgroups: each route against gcm_ref (E.run),
    and the one-pass route bit-equal to its two-pass twin in protect output,
    unprotect statuses, lengths, segment, every exported context, and in
    srtp_stats' roc_rechecks and repaired."""
    outs, gs = [], []
    for name in (kernels + "_fused", kernels + "_two_pass"):
        e = make(engine_factory, ROUTES[name])
        g0 = e.gcm_stats()
        out, n_data = _mixed_run(e, n)
        outs.append(out)
        gs.append(delta(e, g0))
    assert outs[0] == outs[1]
    assert gs[1] == ZERO and gs[0] == {"opened": n_data, "restored": 0, "late": 0}


# --------------------------------------------------- 3. overturned verdicts
def _short_header_packet(mk, ms, seq, n_data):
    """A sealed SRTP packet whose extension length, as received, is -2 words:
    a header length of 8, below the fixed header of 16, so that the SSRC and
    the extension header lie inside the ciphered range.  The receiver takes
    SSRC and header length from the bytes as they come, so the packet is built
    from its ciphertext: the tag over it, under the IV those bytes give."""
    enc, salt = G.derive(mk, ms, False)
    rks = G.expand_key(enc)
    head = bytes([0x90, 96]) + seq.to_bytes(2, "big") + bytes(4)
    ct = bytearray(G.payload(n_data, 900 + seq))
    ct[6:8] = (-2 & 0xFFFF).to_bytes(2, "big")  # bytes 14..16 of the packet
    iv = G.rtp_iv(salt, bytes(ct[0:4]), 0, seq)
    return head + bytes(ct) + G._tag(rks, iv, head, bytes(ct))


def _overturned(e, seed):
    """[(receiver, bytes, flag, tags)] in bundle order, and the earlier bundle.
    tags: "spec" the open pass deciphers it (valid under g0, speculable);
    "undo" the walk refuses it all the same (abort: only under abort-on-error);
    "late" accepted, and deciphered only after the walk; "same" must come out
    byte for byte as it went in."""
    k128, k256 = E.keys(seed), E.keys(seed + 1, 32)
    f128, f256 = E.F(e, True, *k128, E.GCM128), E.F(e, True, *k256, E.GCM256)
    groups = []
    # (a) a packet and its exact copy, (b) a replay from the earlier bundle, (d) DISCARD / SILENCE: GCM-128 SRTP
    snd, rcv = E.T(RTP, f128), E.T(RTP, f128)
    early = E.ref_protect(snd.r, E._stream(0xB1, [5, 6], plen=33))
    a = E.ref_protect(snd.r, E._stream(0xB1, range(10, 22), plen=40))
    g = [(rcv, a[i], 0, {"spec"}) for i in range(5)]
    g += [(rcv, a[5], N.PKT_FLAG_DISCARD, set()), (rcv, a[6], N.PKT_FLAG_SILENCE, set())]
    g += [(rcv, p, 0, {"spec"}) for p in a[7:]]
    g += [(rcv, a[2], 0, {"spec", "undo", "same"}), (rcv, early[0], 0, {"spec", "undo", "same"})]
    groups.append(g)
    prior = [(rcv, p) for p in early]
    # (f) a flipped bit in the data of one packet and in the tag of another: GCM-256 SRTP
    snd, rcv = E.T(RTP, f256), E.T(RTP, f256)
    b = E.ref_protect(snd.r, [G.rtp_packet(0xB2, 30 + i, G.payload(17 + 16 * i, i), csrcs=i % 3) for i in range(10)])
    bad_data, bad_tag = bytearray(b[1]), bytearray(b[2])
    bad_data[30] ^= 0x08
    bad_tag[-4] ^= 0x40
    groups.append([(rcv, b[0], 0, {"spec"}), (rcv, bytes(bad_data), 0, {"same"}), (rcv, bytes(bad_tag), 0, {"same"})] +
                  [(rcv, p, 0, {"spec"}) for p in b[3:]])
    # (c) a malformed packet, then three valid ones of the same transformer
    snd, rcv = E.T(RTP, f128), E.T(RTP, f128)
    c = E.ref_protect(snd.r, E._stream(0xB3, range(40, 45), plen=24))
    bad = E._raw_rtp(0xB3, 60, 0x90, b"\xbe\xde" + (-5 & 0xFFFF).to_bytes(2, "big"), 44)
    groups.append([(rcv, c[0], 0, {"spec"}), (rcv, c[1], 0, {"spec"}), (rcv, bad, 0, {"same"})] +
                  [(rcv, p, 0, {"spec", "abort"}) for p in c[2:]])
    # (g) 65535 -> 0 inside the bundle, on a fresh context: the guess is ROC 0 for all
    snd, rcv = E.T(RTP, f256), E.T(RTP, f256)
    q = [65533, 65534, 2 + 65536, 3 + 65536, 65535, 1 + 65536]
    sealed = dict(zip(sorted(q), E.ref_protect(snd.r, E._stream(0xB4, sorted(q), plen=20))))
    groups.append([(rcv, sealed[x], 0, {"spec"} if x < 65536 else {"late"}) for x in q])
    # (h) a negative extension length and a header length of 8
    rcv = E.T(RTP, f128)
    groups.append([(rcv, _short_header_packet(*k128, 77, 40), 0, {"late"})])
    # GCM SRTCP: valid ones, (a) a copy of the newest (the reference's SRTCP window is only
    # dependable for the index it received last), (e) E = 0
    csnd, crcv = E.T(RTCP, f128), E.T(RTCP, f128)
    cs = E.ref_protect(csnd.r, [G.rtcp_packet(0xB5, G.payload(12 + 8 * i, i)) for i in range(5)])
    enc, salt = G.derive(*k128, True)
    p0 = G.rtcp_packet(0xB5, G.payload(28, 99))
    wb = (40).to_bytes(4, "big")  # E = 0, index 40
    _, tag = G.seal(G.expand_key(enc), G.rtcp_iv(salt, p0[4:8], 40), p0 + wb, b"")
    groups.append([(crcv, p, 0, {"spec"}) for p in cs] + [(crcv, cs[4], 0, {"spec", "undo", "same"}),
                                                          (crcv, p0 + tag + wb, 0, set())])
    # one bundle: the groups dealt round robin, each keeping its order
    items = []
    while any(groups):
        for g in groups:
            if g:
                items.append(g.pop(0))
    return prior, items


@pytest.mark.parametrize("abort", [True, False], ids=["abort", "each"])
def test_overturned_verdicts(eng, eng_noabort, route, abort):
    """Every way the walk overturns what the open pass did, in one bundle of
    about 48 packets: all of it as gcm_ref has it, every refused packet byte for
    byte as it came, and the srtp_gcm_stats delta the construction implies --
    zeros on the two-pass twins."""
    e = eng if abort else eng_noabort
    prior, items = _overturned(e, 600 + 10 * abort)
    assert 40 <= len(items) <= 56
    seg, off, ln, cap = E.pack([p for _, p in prior], room=4)
    _, _, st = E.run(e, [t for t, _ in prior], True, seg, off, ln, cap, abort=abort)
    assert st.tolist() == [0, 0]
    g0, s0 = e.gcm_stats(), e.stats()
    flags = np.array([f for _, _, f, _ in items], np.uint32)
    seg, off, ln, cap = E.pack([p for _, p, _, _ in items], room=4)
    seg2, ln2, st = E.run(e, [t for t, _, _, _ in items], True, seg, off, ln, cap, flags=flags, abort=abort)
    undone = lambda tags: "undo" in tags or (abort and "abort" in tags)
    for i, (_, p, _, tags) in enumerate(items):
        if "same" in tags or undone(tags):
            assert st[i] != 0, (i, tags)
            assert seg2[off[i]:off[i] + len(p)].tobytes() == p, (i, tags, int(st[i]))
        elif tags & {"spec", "late"}:
            assert st[i] == 0, (i, tags, int(st[i]))
    assert sorted(set(st.tolist())) == ([0, 1, 2, 6, 8] if abort else [0, 1, 2, 6])
    # (g): three re-checks; a bundle in which a packet throws under abort-on-error is walked twice
    assert e.stats()["roc_rechecks"] - s0["roc_rechecks"] in ((3, 6) if abort else (3,))
    want = {"opened": sum("spec" in t for _, _, _, t in items),
            "restored": sum("spec" in t and undone(t) for _, _, _, t in items),
            "late": sum("late" in t for _, _, _, t in items)}
    assert want["restored"] == (6 if abort else 3) and want["late"] == 4 and want["opened"] > 25
    assert delta(e, g0) == (want if route.endswith("fused") else ZERO)


# ------------------------------------------------------- 4. the default route
def _sealed_by_engine(e, f, n, seed):
    snd = E.T(RTP, f)
    n_ssrc = max(1, n // 25)
    pk = [G.rtp_packet(0x7400000 + i % n_ssrc, 1 + i // n_ssrc, G.payload(24, (seed + i) % 64)) for i in range(n)]
    seg, off, ln, cap = E.pack(pk, room=16)
    st = e.transform_host(False, snd.tid, seg, off, ln, cap)
    assert st.tolist() == [0] * n
    return pk, seg, off, ln, cap


def test_default_route(engine_factory):
    """No flags.  A bundle of srtp_gcm_wave_max() + 1 packets in which every
    40th copies an earlier one and three carry a flipped bit, one of 64
    packets, and one of srtp_gcm_open_wave_min(): bit for bit what a
    NO_GCM_SPEC engine makes of the same bytes, and `opened` moves exactly
    where the exported limits put the one-pass route."""
    lib = N.lib()
    wmax, lane_min, wave_min, wave_max = (int(lib.srtp_gcm_wave_max()), int(lib.srtp_gcm_open_lane_min()),
                                          int(lib.srtp_gcm_open_wave_min()), int(lib.srtp_gcm_open_wave_max()))
    dflt, twin = E.make_engine(engine_factory), make(engine_factory, N.DEBUG_NO_GCM_SPEC)
    for k, n in enumerate((wmax + 1, 64, wave_min)):
        mk, ms = E.keys(720 + k)
        fs = [E.F(x, True, mk, ms, E.GCM128) for x in (dflt, twin)]
        pk, seg, off, ln, cap = _sealed_by_engine(dflt, fs[0], n, k)
        for i in range(40, n, 40):  # a copy of an earlier packet of the bundle (all of one length)
            src = i - 17
            seg[off[i]:off[i] + ln[i]] = seg[off[src]:off[src] + ln[src]]
        for i, at in ((3, 13), (n // 2 + 1, 20), (n - 2, -1)):
            seg[off[i] + (at if at >= 0 else ln[i] - 1)] ^= 0x10
        outs = []
        for x, f in zip((dflt, twin), fs):
            g0 = x.gcm_stats()
            rcv = E.T(RTP, f)
            s, l = seg.copy(), ln.copy()
            st = x.transform_host(True, rcv.tid, s, off, l, cap)
            ex = sorted((ssrc, sorted(stt.items())) for ssrc, stt in x.export_contexts(rcv.e).items())
            outs.append((st.tolist(), l.tolist(), s.tobytes(), ex))
            d = delta(x, g0)
            fused = x is dflt and (n >= lane_min if n > wmax else wave_min <= n <= wave_max)
            assert (d["opened"] > 0) == fused, (n, d)
            if fused:
                assert d["restored"] == sum(1 for v in st.tolist() if v == 1)
            else:
                assert d == ZERO
        assert outs[0] == outs[1]
        st = outs[0][0]
        assert st.count(1) == len(range(40, n, 40)) and st.count(2) == 3 and st.count(0) == n - st.count(1) - 3


# ----------------------------------------------------------- 5. untouched paths
@pytest.mark.parametrize("n", [1, 8])
def test_small_bundles_stay_on_k_small(engine_factory, n):
    e = E.make_engine(engine_factory)
    snd, rcv = E.sender_receiver(e, RTP, E.GCM128, 730 + n)
    g0, s0 = e.gcm_stats(), e.stats()["small_aead_bundles"]
    pk = E._stream(0xB8, range(3, 3 + n), plen=30)
    seg, off, ln, cap = E.pack(pk)
    seg2, ln2, st = E.run(e, snd, False, seg, off, ln, cap)
    _, _, st2 = E.run(e, rcv, True, seg2, off, ln2, cap)
    assert st.tolist() == [0] * n and st2.tolist() == [0] * n
    assert e.stats()["small_aead_bundles"] == s0 + 2 and delta(e, g0) == ZERO
    # the flag does not change which bundles k_small takes
    e.set_debug(N.DEBUG_NO_GCM_SPEC)
    try:
        seg, off, ln, cap = E.pack(E._stream(0xB8, range(20, 20 + n), plen=30))
        E.run(e, snd, False, seg, off, ln, cap)
        assert e.stats()["small_aead_bundles"] == s0 + 3
    finally:
        e.set_debug(0)


def test_protect_is_untouched(eng):
    snd, _ = E.sender_receiver(eng, RTP, E.GCM256, 740)
    csnd, _ = E.sender_receiver(eng, RTCP, E.GCM128, 741)
    g0 = eng.gcm_stats()
    items = [(snd, p) for p in E._stream(0xB9, range(1, 21), plen=25)]
    items += [(csnd, G.rtcp_packet(0xBA, G.payload(20, i))) for i in range(6)]
    seg, off, ln, cap = E.pack([p for _, p in items], room=24)
    _, _, st = E.run(eng, [t for t, _ in items], False, seg, off, ln, cap)
    assert st.tolist() == [0] * len(items) and delta(eng, g0) == ZERO


@pytest.mark.parametrize("aead", [False, True], ids=["plain", "switch_on"])
def test_engines_without_gcm_key_sets_report_zeros(engine_factory, aead):
    e = engine_factory(max_contexts=4096, max_factories=16, max_transformers=16)
    if aead:
        e.enable_aead()
    f = E.F(e, True, *E.keys(750, 16, 14), *E.P80)
    s, r = E.T(RTP, f), E.T(RTP, f)
    pk = [G.rtp_packet(0x750 + (i % 3), 9 + i, G.payload(10 + 7 * i, i)) for i in range(20)]
    seg, off, ln, cap = E.pack(pk)
    seg2, ln2, _ = E.run(e, s, False, seg, off, ln, cap)
    pk2 = bytearray(seg2)
    pk2[int(off[4]) + 15] ^= 1
    _, _, st = E.run(e, r, True, np.frombuffer(bytes(pk2), np.uint8).copy(), off, ln2, cap)
    assert st[4] == 2 and e.gcm_stats() == ZERO


def test_dispatcher_sums_the_shards():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    d = SRTPDispatcher([0, 0], max_contexts=4096, max_factories=16, max_transformers=16)
    try:
        d.enable_aead()
        lib = N.lib()
        per = []
        for i in range(2):
            h = C.c_void_p(lib.srtp_dispatch_engine(d.h, i))
            assert lib.srtp_engine_set_debug(h, N.DEBUG_NO_GCM_WAVE | N.DEBUG_FORCE_GCM_SPEC) == 0
            per.append(h)
        f = E.F(d, True, *E.keys(760), E.GCM128)
        snd, rcv = E.T(RTP, f), E.T(RTP, f)
        pk = [G.rtp_packet(0x760 + (i % 8), 3 + i // 8, G.payload(16 + i % 7, i)) for i in range(48)]
        assert len({d.shard_of(0x760 + s) for s in range(8)}) == 2
        seg, off, ln, cap = E.pack(pk, room=24)
        seg2, ln2, st = E.run(d, snd, False, seg, off, ln, cap, transform=d.transform_host)
        seg2[off[47]:off[47] + ln2[46]] = seg2[off[46]:off[46] + ln2[46]]  # a copy: the same stream, a replay
        ln2[47] = ln2[46]
        _, _, st = E.run(d, rcv, True, seg2, off, ln2, cap, transform=d.transform_host)
        assert st.tolist() == [0] * 47 + [1]
        shards = []
        for h in per:
            g = N.GcmStats()
            assert lib.srtp_engine_gcm_stats(h, C.byref(g)) == 0
            shards.append(g.as_dict())
        assert all(s["opened"] > 0 for s in shards)
        total = d.gcm_stats()
        assert total == {k: shards[0][k] + shards[1][k] for k in total}
        assert total == {"opened": 48, "restored": 1, "late": 0}
    finally:
        d.close()
