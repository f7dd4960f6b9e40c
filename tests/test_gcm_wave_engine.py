"""The engine's AES-GCM passes a wave per packet (k_gcm_wave), reached on every
bundle size through SRTP_DEBUG_FORCE_GCM_WAVE, against tests/gcm_ref.py and
against the lane kernel (SRTP_DEBUG_NO_GCM_WAVE) on identical inputs:
statuses, lengths, every byte of the segment and the exported context state.
The cases are test_gcm_engine.py's, run on engines that carry the flags, plus
bundles that mix AES_CM_128_HMAC_SHA1_80 and GCM key sets and skipped packets
(waves and workgroups without GCM work), and the default route on either side
of its size limit."""
import numpy as np
import pytest

import gcm_ref as G
import test_gcm_engine as E
from libjitsi_amd import _native as N
from libjitsi_amd import srtp

pytestmark = pytest.mark.gpu

RTP, RTCP = E.RTP, E.RTCP
ROUTES = {"wave": N.DEBUG_FORCE_GCM_WAVE, "lane": N.DEBUG_NO_GCM_WAVE}


def make(engine_factory, flags, **kw):
    e = E.make_engine(engine_factory, **kw)
    e.set_debug(flags)
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


def test_golden(eng):
    E.test_golden(eng)


@pytest.mark.parametrize("pol", [E.GCM128, E.GCM256], ids=["128", "256"])
def test_lengths(eng, pol):
    E.test_lengths(eng, pol)


@pytest.mark.parametrize("abort", [False, True], ids=["each", "abort"])
def test_reject_shapes(eng, eng_noabort, abort):
    """Among them the single 8-byte SRTCP packet and the capacities around 16 and 20."""
    E.test_reject_shapes(eng, eng_noabort, abort)


def test_tampering(eng):
    E.test_tampering(eng)


def test_state(eng):
    """Among it DISCARD / SILENCE, and a ROC the walk overturns: gcm_reverify
    reads the S that the verify pass of this route wrote."""
    E.test_state(eng)


def test_srtcp_e0(eng):
    E.test_srtcp_e0(eng)


def _mixed(e, n):
    """n packets over GCM-128 / GCM-256 SRTP, GCM SRTCP and AES-CM + HMAC
    streams, every seventh one flagged SKIP, and runs of four and more
    consecutive non-GCM packets (whole workgroups of k_gcm_wave without work)."""
    fg, fh = E.F(e, True, *E.keys(700), E.GCM128), E.F(e, True, *E.keys(701, 32), E.GCM256)
    fa = E.F(e, True, *E.keys(702, 16, 14), *E.P80)
    pairs = [(E.T(RTP, f), E.T(RTP, f)) for f in (fg, fh, fa)] + [(E.T(RTCP, fg), E.T(RTCP, fg)),
                                                                  (E.T(RTCP, fa), E.T(RTCP, fa))]
    items, flags = [], []
    for i in range(n):
        k = 2 if (i // 6) % 3 == 1 else (i * 7 + i // 5) % 5  # runs of six AES-CM packets
        s, r = pairs[k]
        if s.kind == RTP:
            p = G.rtp_packet(0x7000 + 16 * k + i % 3, 5 + i // 3, G.payload((i * 13) % 70, i), ext_words=i % 2 - 1)
        else:
            p = G.rtcp_packet(0x7100 + 16 * k + i % 2, G.payload(8 + 4 * (i % 9), i))
        items.append((s, r, p))
        flags.append(N.PKT_FLAG_SKIP if i % 7 == 3 else 0)
    return items, np.array(flags, np.uint32)


@pytest.mark.parametrize("n", [1, 4, 5, 300])
def test_mixed_bundle_both_routes(engine_factory, n):
    """The same bundle on a FORCE_GCM_WAVE and a NO_GCM_WAVE engine: each
    against gcm_ref (E.run), and the two bit-equal in status, length, segment
    and every exported context."""
    outs = []
    for name, fl in ROUTES.items():
        e = make(engine_factory, fl)
        items, flags = _mixed(e, n)
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
        outs.append((st.tolist(), ln2.tolist(), seg2.tobytes(), st3.tolist(), ln3.tolist(), seg3.tobytes(), ex))
    assert outs[0] == outs[1]


def test_default_route(engine_factory):
    """No flags: a bundle of srtp_gcm_wave_max() packets and one of one more --
    the two sides of launch_gcm's size rule -- both match the reference.  The
    limit is in the thousands, so the reference here is the host AEAD
    (srtp_aes_gcm) under the session key and IV of RFC 7714, packet by packet,
    and the unprotect is held to the plaintext it started from."""
    e = E.make_engine(engine_factory)
    wmax = int(N.lib().srtp_gcm_wave_max())
    for k, n in enumerate((wmax, wmax + 1)):
        if n == 0:
            continue
        mk, ms = E.keys(710 + k)
        f = E.F(e, True, mk, ms, E.GCM128)
        snd, rcv = E.T(RTP, f), E.T(RTP, f)
        enc, salt = G.derive(mk, ms, False)
        n_ssrc = max(1, n // 25)
        pk = [G.rtp_packet(0x7300000 + i % n_ssrc, 1 + i // n_ssrc, G.payload(17 + i % 23, i % 64)) for i in range(n)]
        seg, off, ln, cap = E.pack(pk, room=16)
        seg2, ln2 = seg.copy(), ln.copy()
        st = e.transform_host(False, snd.tid, seg2, off, ln2, cap)
        assert st.tolist() == [0] * n and np.array_equal(ln2, ln + 16)
        for i, p in enumerate(pk):
            c, t = srtp.aes_gcm(enc, G.rtp_iv(salt, p[8:12], 0, 1 + i // n_ssrc), p[:12], p[12:])
            assert seg2[off[i]:off[i] + ln2[i]].tobytes() == p[:12] + c + t, i
        seg3, ln3 = seg2.copy(), ln2.copy()
        st = e.transform_host(True, rcv.tid, seg3, off, ln3, cap)
        assert st.tolist() == [0] * n and np.array_equal(ln3, ln)
        for i, p in enumerate(pk):
            assert seg3[off[i]:off[i] + ln3[i]].tobytes() == p, i
