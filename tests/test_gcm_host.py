"""RFC 7714 AES-GCM profiles, host side (no GPU): the engine's own GF(2^128)
arithmetic (srtp_aes_gcm, which also builds the GPU path's GHASH tables), the
test-side reference (tests/gcm_ref.py) and OpenSSL pinned to each other; the
RFC 7714 key derivation; the DTLS-SRTP profile table; the dispatcher's
may-throw test; and the OpenSSL-sealed golden fixture replayed through the
reference."""
import json
import os

import numpy as np
import pytest

import gcm_ref as G
from libjitsi_amd import _native as N
from libjitsi_amd import dtls, profile_policies, srtp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcm_rfc7714.json")

# key, plaintext, ciphertext, tag (IV = 0^96, no AAD); confirmed with OpenSSL
KATS = [(bytes(16), b"", "", "58e2fccefa7e3061367f1d57a4e7455a"),
        (bytes(16), bytes(16), "0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf"),
        (bytes(32), b"", "", "530f8afbc74536b9a963b4f1c4cb738b"),
        (bytes(32), bytes(16), "cea7403d4d606b6e074ec5d3baf39d18", "d0d1c8a799996bf0265b98b5d48ab919")]


@pytest.mark.parametrize("key,pt,ct,tag", KATS)
def test_known_answers_reference(key, pt, ct, tag):
    c, t = G.seal(G.expand_key(key), bytes(12), b"", pt)
    assert (c.hex(), t.hex()) == (ct, tag)
    assert G.open_(G.expand_key(key), bytes(12), b"", c, t) == pt


@pytest.mark.parametrize("key,pt,ct,tag", KATS)
def test_known_answers_engine_host(key, pt, ct, tag):
    c, t = srtp.aes_gcm(key, bytes(12), b"", pt)
    assert (c.hex(), t.hex()) == (ct, tag)
    assert srtp.aes_gcm(key, bytes(12), b"", c, t) == pt


def test_known_answers_openssl():
    if not G.have_openssl():
        pytest.skip("libcrypto not found")
    for key, pt, ct, tag in KATS:
        c, t = G.openssl_gcm(key, bytes(12), b"", pt)
        assert (c.hex(), t.hex()) == (ct, tag)


def _flip(b: bytes, bit: int) -> bytes:
    x = bytearray(b)
    x[(bit // 8) % len(x)] ^= 1 << (bit % 8)
    return bytes(x)


def test_random_cross_check():
    """gcm_ref, srtp_aes_gcm and OpenSSL on seeded random cases: every AAD and
    data length of the list with both key sizes (108 cases), seal, open, and
    open with one flipped bit in each of AAD, data and tag."""
    ssl = G.have_openssl()
    rng = np.random.default_rng(7714)
    n = 0
    for klen in (16, 32):
        for alen in (0, 8, 12, 16, 28, 33):
            for dlen in (0, 1, 15, 16, 17, 31, 32, 33, 1188):
                key, iv = rng.bytes(klen), rng.bytes(12)
                aad, data = rng.bytes(alen), rng.bytes(dlen)
                rks = G.expand_key(key)
                c, t = srtp.aes_gcm(key, iv, aad, data)
                assert G.seal(rks, iv, aad, data) == (c, t)
                assert G.open_(rks, iv, aad, c, t) == data
                if ssl:
                    assert G.openssl_gcm(key, iv, aad, data) == (c, t)
                    assert G.openssl_gcm(key, iv, aad, c, t) == data
                assert srtp.aes_gcm(key, iv, aad, c, t) == data
                bit = int(rng.integers(0, 1 << 16))
                bad = [(aad, c, _flip(t, bit))]
                if alen:
                    bad.append((_flip(aad, bit), c, t))
                if dlen:
                    bad.append((aad, _flip(c, bit), t))
                for a2, c2, t2 in bad:
                    assert srtp.aes_gcm(key, iv, a2, c2, t2) is None
                    assert G.open_(rks, iv, a2, c2, t2) is None
                    if ssl:
                        assert G.openssl_gcm(key, iv, a2, c2, t2) is None
                n += 1
    assert n == 108


def test_open_leaves_data_untouched_on_mismatch():
    import ctypes as C
    key, iv = bytes(range(16)), bytes(range(12))
    c, t = srtp.aes_gcm(key, iv, b"hdr", b"some plaintext bytes")
    buf = (C.c_uint8 * len(c)).from_buffer_copy(c)
    tag = (C.c_uint8 * 16).from_buffer_copy(_flip(t, 5))
    assert N.lib().srtp_aes_gcm(1, key, 16, iv, b"hdr", 3, buf, len(c), tag) == 1
    assert bytes(buf) == c
    assert N.lib().srtp_aes_gcm(1, key, 24, iv, b"hdr", 3, buf, len(c), tag) == -1  # SRTP_EINVAL


def _pol(p):
    return (p.encType, p.encKeyLength, p.authType, p.authKeyLength, p.authTagLength, p.saltKeyLength)


def test_policy_table():
    for name, klen in (("AEAD_AES_128_GCM", 16), ("AEAD_AES_256_GCM", 32)):
        assert [_pol(p) for p in profile_policies(name)] == [G.policy(klen)] * 2 == [(5, klen, 0, 0, 16, 12)] * 2
    assert (N.AESGCM_ENCRYPTION, N.PROFILE_AEAD_AES_128_GCM, N.PROFILE_AEAD_AES_256_GCM) == (5, 7, 8)
    assert srtp.SRTPPolicy.AESGCM_ENCRYPTION == 5


def test_dtls_table_is_unchanged():
    """The four DTLS-SRTP ids answer as before; the AEAD ids stay unknown to
    srtp_dtls_profile_keys until the engine runs the profile."""
    import ctypes as C
    want = {0x0001: (1, 16, 1, 20, 10, 14, 10), 0x0002: (1, 16, 1, 20, 4, 14, 10),
            0x0005: (0, 0, 1, 20, 10, 0, 10), 0x0006: (0, 0, 1, 20, 4, 0, 10)}
    assert dtls.PROFILES == tuple(want)
    for pid, (enc, klen, auth, alen, tag, slen, rtcp_tag) in want.items():
        k = dtls.profile_keys(pid)
        assert _pol(k["srtpPolicy"]) == (enc, klen, auth, alen, tag, slen)
        assert _pol(k["srtcpPolicy"]) == (enc, klen, auth, alen, rtcp_tag, slen)
        assert k["keying_material_len"] == 2 * (klen + slen)
    for pid in (0, 3, 4, 7, 8, 9, 0x0107):
        assert N.lib().srtp_dtls_profile_keys(pid, None, 0, C.byref(N.DtlsKeys())) == -5


@pytest.mark.parametrize("klen", [16, 32])
@pytest.mark.parametrize("rtcp", [False, True])
def test_kdf(klen, rtcp):
    mk, ms = G.payload(klen, 11 + klen), G.payload(12, 12 + klen)
    enc, auth, salt = srtp.derive_session_keys_for(N.AESGCM_ENCRYPTION, mk, ms, rtcp)
    r_enc, r_salt = G.derive(mk, ms, rtcp)
    assert len(r_salt) == 12 and len(r_enc) == klen
    assert enc == r_enc and salt[:12] == r_salt and salt[12:] == b"\0\0" and auth == bytes(20)
    # RFC 7714 11: the same PRF as the AES-CM profile of that key size over the zero-padded salt
    cm_enc, _, cm_salt = srtp.derive_session_keys_for(N.AESCM_ENCRYPTION, mk, ms + b"\0\0", rtcp)
    assert enc == cm_enc and salt[:12] == cm_salt[:12]


def _may_throw(kind, reverse, pkt: bytes, cap=None, flags=0, mask=1 << 16):
    cap = cap or len(pkt) + 20
    buf = bytes(pkt) + bytes(cap - len(pkt)) if cap > len(pkt) else bytes(pkt[:cap])
    return N.lib().srtp_packet_may_throw(kind, int(reverse), buf, len(pkt), cap, flags, mask)


def test_may_throw_covers_the_gcm_malformed_shapes():
    """srtp_packet_may_throw with tag_mask = 1 << 16 answers 1 for every packet
    shape the GCM rules report as ERR_MALFORMED (gcm_ref's, run here)."""
    shapes = []
    ext_past = bytearray(G.rtp_packet(1, 1, b"", 0, 0))[:14]           # extension length past cap
    shapes.append((0, bytes(ext_past) + bytes(1), 15))
    neg = bytearray(G.rtp_packet(1, 2, bytes(40), 0, 0))
    neg[14:16] = (0x10000 - 5).to_bytes(2, "big")                        # negative header length
    shapes.append((0, bytes(neg), None))
    for pad in (4, 16, 20, 32):                                          # header longer than the packet,
        long_hdr = bytearray(G.rtp_packet(1, 3, bytes(8), 1, 0))         # by 16 k and by other amounts
        long_hdr[18:20] = ((8 + pad) // 4).to_bytes(2, "big")
        shapes.append((0, bytes(long_hdr), None))
    hits = 0
    for pkt_kind, pkt, cap in shapes:
        for reverse in (False, True):
            for flags in (0, N.PKT_FLAG_DISCARD):
                f = G.Factory(True, bytes(16), bytes(12), G.policy(16), G.policy(16))
                t = G.Transformer(pkt_kind, f, f)
                c = cap or len(pkt) + 20
                buf = bytearray(pkt[:c] + bytes(max(0, c - len(pkt))))
                st, _ = G.process_one(t, reverse, buf, len(pkt), c, flags)
                if st == 6:
                    hits += 1
                    assert _may_throw(pkt_kind, reverse, pkt, cap, flags) == 1, (pkt.hex(), reverse, flags)
    assert hits == 2 + 4 + 4 * 2  # the first on unprotect, the second both ways, the long headers on protect
    # all three RTP shapes are malformed on protect; the first two on unprotect as well
    f = G.Factory(True, bytes(16), bytes(12), G.policy(16), G.policy(16))
    assert G.process_one(G.Transformer(0, f, f), False, bytearray(shapes[2][1] + bytes(20)), len(shapes[2][1]),
                         len(shapes[2][1]) + 20, 0)[0] == 6
    assert G.process_one(G.Transformer(0, f, f), True, bytearray(shapes[1][1] + bytes(20)), len(shapes[1][1]),
                         len(shapes[1][1]) + 20, N.PKT_FLAG_DISCARD)[0] == 6
    # SRTCP unprotect: shorter than tag + index word
    for L in range(12, 20):
        pkt = G.rtcp_packet(5, bytes(L - 8))
        t = G.Transformer(1, f, f)
        assert G.process_one(t, True, bytearray(pkt + bytes(20)), L, L + 20, 0)[0] == 6
        assert _may_throw(1, True, pkt) == 1


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["streams"]


def test_golden_fixture_through_reference():
    """The OpenSSL-sealed packets: gcm_ref protects to the same bytes and
    unprotects them back (so reference and fixture agree before the GPU test
    holds the engine to the fixture)."""
    streams = _golden()
    assert sum(len(s["packets"]) for s in streams) >= 24
    for s in streams:
        key, salt, pol = bytes.fromhex(s["key"]), bytes.fromhex(s["salt"]), tuple(s["policy"])
        f = G.Factory(True, key, salt, pol, pol)
        snd, rcv = G.Transformer(s["kind"], f, f), G.Transformer(s["kind"], f, f)
        ins = [bytes.fromhex(p["in"]) for p in s["packets"]]
        outs = [bytes.fromhex(p["out"]) for p in s["packets"]]
        seg, off, ln, cap = G.pack(ins)
        st = G.process(snd, False, seg, off, ln, cap)
        assert st.tolist() == [0] * len(ins)
        for i, want in enumerate(outs):
            assert seg[off[i]:off[i] + ln[i]].tobytes() == want, (s["kind"], i)
        st = G.process(rcv, True, seg, off, ln, cap)
        assert st.tolist() == [0] * len(ins)
        for i, want in enumerate(ins):
            assert seg[off[i]:off[i] + ln[i]].tobytes() == want


def test_golden_generator_is_reproducible(tmp_path):
    """tools/make_gcm_golden.py regenerates the committed fixture (with OpenSSL)."""
    if not G.have_openssl():
        pytest.skip("libcrypto not found")
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_gcm_golden", os.path.join(root, "tools", "make_gcm_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.OUT = str(tmp_path / "g.json")
    m.main()
    with open(m.OUT) as a, open(GOLDEN) as b:
        assert json.load(a) == json.load(b)


@pytest.mark.gpu
def test_engine_still_refuses_the_gcm_policy(engine_factory):
    """The engine has no kernel for AES-GCM yet: a factory of that policy
    answers SRTP_EPOLICY, with a 12- or a 14-byte salt."""
    from libjitsi_amd import SRTPContextFactory, SRTPPolicy
    e = engine_factory(max_contexts=1024, max_factories=8, max_transformers=8)
    pol = SRTPPolicy(*G.policy(16))
    with pytest.raises(N.SrtpError) as err:
        SRTPContextFactory(True, bytes(16), bytes(12), pol, pol, engine=e)
    assert "SRTP_EPOLICY" in str(err.value)
    with pytest.raises(N.SrtpError):
        SRTPContextFactory(True, bytes(32), bytes(14), SRTPPolicy(*G.policy(32)), SRTPPolicy(*G.policy(32)), engine=e)
