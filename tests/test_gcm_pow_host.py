"""The host arithmetic the wave-per-packet GCM kernels rest on (no GPU): the
general GF(2^128) product (srtp_gf128_mul), the powers of the hash key
(srtp_gcm_hpowers), GHASH as a sum over those powers 64 blocks at a time, and
the per-packet paths' trailer room."""
import numpy as np

import gcm_ref as G
from libjitsi_amd import _native as N
from libjitsi_amd import srtp

R = 0xE1 << 120
ONE = bytes([0x80]) + bytes(15)  # the field's 1 in GCM's bit order
ONES = bytes([0xFF]) * 16


def mul(x: bytes, y: bytes) -> bytes:
    """SP 800-38D algorithm 1, restated."""
    xi, v, z = int.from_bytes(x, "big"), int.from_bytes(y, "big"), 0
    for i in range(128):
        if (xi >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ R if v & 1 else v >> 1
    return z.to_bytes(16, "big")


def xor(a: bytes, b: bytes) -> bytes:
    return bytes(p ^ q for p, q in zip(a, b))


def ghash_serial(h: bytes, blocks) -> bytes:
    y = bytes(16)
    for x in blocks:
        y = mul(xor(y, x), h)
    return y


def ghash_chunks(pw, blocks) -> bytes:
    """What k_gcm_wave computes: per chunk of m <= 64 blocks, block l (block 0
    with the running value XORed in) times H^(m - l), XORed together."""
    z = bytes(16)
    for base in range(0, len(blocks), 64):
        chunk = blocks[base:base + 64]
        m, acc = len(chunk), bytes(16)
        for l, x in enumerate(chunk):
            acc = xor(acc, srtp.gf128_mul(xor(x, z) if l == 0 else x, pw[m - l - 1]))
        z = acc
    return z


def test_gf128_mul():
    rng = np.random.default_rng(128)
    h = rng.bytes(16)
    edge = [bytes(16), ONE, h, ONES]
    ops = [(a, b) for a in edge for b in edge] + [(rng.bytes(16), rng.bytes(16)) for _ in range(64)]
    for a, b in ops:
        assert srtp.gf128_mul(a, b) == mul(a, b)
        assert srtp.gf128_mul(a, b) == srtp.gf128_mul(b, a)
    for a in edge + [rng.bytes(16)]:
        assert srtp.gf128_mul(a, ONE) == a
        assert srtp.gf128_mul(a, bytes(16)) == bytes(16)


def test_ghash_from_powers_is_gcm_refs():
    """The packet's one list of blocks -- AAD, data, lengths -- summed from the
    powers is gcm_ref's GHASH, for a 1200-byte packet and the odd shapes."""
    rng = np.random.default_rng(7)
    h = rng.bytes(16)
    pw = srtp.gcm_hpowers(h)
    for alen, dlen in ((12, 1188), (0, 0), (1, 1), (28, 975), (1030, 33), (12, 4100)):
        aad, ct = rng.bytes(alen), rng.bytes(dlen)
        blocks = [part[o:o + 16].ljust(16, b"\0") for part in (aad, ct) for o in range(0, len(part), 16)]
        blocks.append((alen * 8).to_bytes(8, "big") + (dlen * 8).to_bytes(8, "big"))
        assert ghash_chunks(pw, blocks) == G.ghash(int.from_bytes(h, "big"), aad, ct).to_bytes(16, "big")


def test_hpowers():
    rng = np.random.default_rng(64)
    for h in (rng.bytes(16), ONE, ONES, bytes(16)):
        pw = srtp.gcm_hpowers(h)
        assert len(pw) == 64 and pw[0] == h
        p = h
        for k in range(1, 64):
            p = mul(p, h)
            assert pw[k] == p, k


def test_ghash_from_powers():
    rng = np.random.default_rng(65)
    h = rng.bytes(16)
    pw = srtp.gcm_hpowers(h)
    for n in (1, 63, 64, 65, 128, 129):
        blocks = [rng.bytes(16) for _ in range(n)]
        assert ghash_chunks(pw, blocks) == ghash_serial(h, blocks), n


def test_room_and_symbols():
    L = N.lib()
    assert L.srtp_trailer_room(0) == 16
    for v in (1, 2, -1, 255, 1 << 30, -(1 << 31)):
        assert L.srtp_trailer_room(v) == 20
    assert L.srtp_engine_trailer_room(None) == 16
    assert L.srtp_aggregator_trailer_room(None) == 16
    for sym in ("srtp_aes_gcm_device_ex", "srtp_gcm_wave_max"):
        assert getattr(L, sym)
    assert L.srtp_gf128_mul(None, bytes(16), (N.C.c_uint8 * 16)()) == -1
    assert N.DEBUG_NO_GCM_WAVE == 0x10 and N.DEBUG_FORCE_GCM_WAVE == 0x20
