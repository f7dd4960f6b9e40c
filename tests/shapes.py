"""Deterministic grids of packet shapes for the parity tests (a helper, imported
like harness.py).

libjitsi_amd/synth.py draws payload lengths at random, writes RTP headers of 12
or 20 bytes only and rounds every SRTCP length to a multiple of 4.  The grids
here walk what that leaves out, one packet per cell:

rtp_grid    12 header shapes (CSRC lists, extensions of 0..5 words: headers of
            12..92 bytes, the payload starting at 0, 4, 8 and 12 mod 16) x 74
            payload lengths (0..69: every residue of the payload mod 32 and of
            the MAC input mod 64; 111..113 and 1188 for the longer loops).
rtcp_grid   every length 8..139 and 1187..1190: each residue of L mod 4 (the
            trailer at an odd offset), of the MAC input mod 64, and the
            reference's DROP_INVALID lengths 8..11.
quirk_grid  first bytes and extension length fields whose header comes out
            longer than the packet, shorter than 12 bytes or negative (the
            reference reads the field as a signed 16-bit number), at lengths
            that put the payload at -32..+4 bytes and the field past the end.

All builders return synth.Bundle objects laid out by synth.layout (16-byte
aligned regions, 16 bytes of room).  The bytes between a packet's end and the
next region are random, not zero, so a read or a write past `len` shows up in a
whole-segment comparison.
"""
from __future__ import annotations

import numpy as np

from libjitsi_amd import synth

# (CC, extension words; -1: no X bit)
HEADER_SHAPES = ((0, -1), (1, -1), (2, -1), (3, -1), (15, -1), (0, 0), (0, 1), (0, 2), (0, 3),
                 (1, 2), (2, 5), (15, 4))
RTP_PAYLOADS = tuple(range(70)) + (111, 112, 113, 1188)
RTP_N = len(HEADER_SHAPES) * len(RTP_PAYLOADS)  # 888
RTP_SSRCS = 11
RTCP_LENGTHS = tuple(range(8, 140)) + (1187, 1188, 1189, 1190)  # 136
RTCP_SSRCS = 7
# (byte 0, extension length field or None)
QUIRKS = ((0x8F, None), (0x9F, 0), (0x90, 0xFFFF), (0x90, 0xFFFD), (0x90, 0xFFFC), (0x90, 0x8000),
          (0x90, 0x7FFF), (0x90, 0x0010), (0x92, 0xFFFE))
QUIRK_LENGTHS = (12, 13, 14, 15, 16, 20, 24, 40, 56, 60, 64, 68, 72, 76, 80, 96)  # x 9 = 144
QUIRK_SSRCS = 5


def header_len(cc: int, ext_words: int) -> int:
    return 12 + 4 * cc + (4 + 4 * ext_words if ext_words >= 0 else 0)


def _be32(seg, o, v):
    v = np.asarray(v, np.uint32)
    for k in range(4):
        seg[o + k] = ((v >> (24 - 8 * k)) & 0xFF).astype(np.uint8)


def _bundle(rng, length, ssrc, seq):
    """A bundle of random bytes with the given lengths; the callers write the
    fixed header fields over it."""
    length = np.asarray(length, np.uint32)
    off, cap, total = synth.layout(length)
    seg = rng.integers(0, 256, total, dtype=np.uint8)
    return synth.Bundle(seg, off, length, cap, np.zeros(len(length), np.uint32),
                        np.asarray(ssrc, np.uint32), np.asarray(seq, np.uint32), {})


def _rtp_grid_once(rng, ssrc_base):
    idx = np.arange(RTP_N, dtype=np.int64)
    cc = np.repeat([s[0] for s in HEADER_SHAPES], len(RTP_PAYLOADS))
    ext = np.repeat([s[1] for s in HEADER_SHAPES], len(RTP_PAYLOADS))
    pay = np.tile(RTP_PAYLOADS, len(HEADER_SHAPES))
    hlen = 12 + 4 * cc + np.where(ext >= 0, 4 + 4 * ext, 0)
    ssrc = (ssrc_base + idx % RTP_SSRCS).astype(np.uint32)
    seq = ((65500 + idx // RTP_SSRCS) & 0xFFFF).astype(np.uint32)
    b = _bundle(rng, hlen + pay, ssrc, seq)
    o = b.off.astype(np.int64)
    b.seg[o] = (0x80 | cc | np.where(ext >= 0, 0x10, 0) | np.where(idx % 7 == 0, 0x20, 0)).astype(np.uint8)
    b.seg[o + 1] = (96 | np.where(idx % 5 == 0, 0x80, 0)).astype(np.uint8)
    b.seg[o + 2] = (seq >> 8).astype(np.uint8)
    b.seg[o + 3] = (seq & 0xFF).astype(np.uint8)
    _be32(b.seg, o + 4, (seq.astype(np.uint64) * 3000) & 0xFFFFFFFF)
    _be32(b.seg, o + 8, ssrc)
    x = ext >= 0  # the extension's length field; its profile word, data and the CSRCs stay random
    ox = o[x] + 12 + 4 * cc[x]
    b.seg[ox + 2] = (ext[x] >> 8).astype(np.uint8)
    b.seg[ox + 3] = (ext[x] & 0xFF).astype(np.uint8)
    b.meta.update(cc=cc, ext=ext, payload=pay, header=hlen)
    return b


def rtp_grid(seed: int, ssrc_base: int = 0x1000, reps: int = 1) -> synth.Bundle:
    """Every header shape x every payload length, shape-major.  Packet i of a
    repetition has SSRC ssrc_base + i % 11 and sequence 65500 + i // 11 (every
    context crosses the ROC wrap), P on every 7th packet and M on every 5th.
    Repetition r uses ssrc_base + 16 * r and fresh random bytes."""
    rng = np.random.default_rng(seed)
    parts = [_rtp_grid_once(rng, ssrc_base + 16 * r) for r in range(reps)]
    if reps == 1:
        return parts[0]
    b = synth.concat(parts)
    b.meta = {k: np.concatenate([p.meta[k] for p in parts]) for k in parts[0].meta}
    return b


def rtcp_grid(seed: int, ssrc_base: int = 0x2000) -> synth.Bundle:
    """One RTCP packet of every length in RTCP_LENGTHS: V = 2, PT 200..204, the
    length field as synth.rtcp_bundle writes it, SSRC ssrc_base + i % 7."""
    rng = np.random.default_rng(seed)
    length = np.array(RTCP_LENGTHS, np.int64)
    idx = np.arange(len(length), dtype=np.int64)
    ssrc = (ssrc_base + idx % RTCP_SSRCS).astype(np.uint32)
    b = _bundle(rng, length, ssrc, np.zeros(len(length), np.uint32))
    o = b.off.astype(np.int64)
    words = (length // 4 - 1).astype(np.uint32)
    b.seg[o] = 0x80
    b.seg[o + 1] = (200 + idx % 5).astype(np.uint8)
    b.seg[o + 2] = (words >> 8).astype(np.uint8)
    b.seg[o + 3] = (words & 0xFF).astype(np.uint8)
    _be32(b.seg, o + 4, ssrc)
    return b


def quirk_grid(seed: int, ssrc_base: int = 0x3000) -> synth.Bundle:
    """QUIRKS x QUIRK_LENGTHS, quirk-major: RTP packets whose first byte and
    extension length field give a header longer than the packet, shorter than
    12 bytes or negative.  The field is written only where it lies inside the
    packet; elsewhere the reference reads the random bytes behind it."""
    rng = np.random.default_rng(seed)
    n = len(QUIRKS) * len(QUIRK_LENGTHS)
    idx = np.arange(n, dtype=np.int64)
    length = np.tile(QUIRK_LENGTHS, len(QUIRKS))
    ssrc = (ssrc_base + idx % QUIRK_SSRCS).astype(np.uint32)
    seq = (100 + idx // QUIRK_SSRCS).astype(np.uint32)
    b = _bundle(rng, length, ssrc, seq)
    o = b.off.astype(np.int64)
    b.seg[o] = np.repeat([q[0] for q in QUIRKS], len(QUIRK_LENGTHS)).astype(np.uint8)
    b.seg[o + 1] = 96
    b.seg[o + 2] = (seq >> 8).astype(np.uint8)
    b.seg[o + 3] = (seq & 0xFF).astype(np.uint8)
    _be32(b.seg, o + 8, ssrc)
    for i in range(n):
        b0, field = QUIRKS[i // len(QUIRK_LENGTHS)]
        at = 12 + 4 * (b0 & 0x0F) + 2
        if field is not None and at + 1 < int(length[i]):
            b.seg[o[i] + at] = field >> 8
            b.seg[o[i] + at + 1] = field & 0xFF
    return b


def tamper_positions(lengths):
    """{packet: byte offset} of tamper(): every third packet, the offset cycling
    through byte 1 (fixed header), 5, 12 (CSRC / extension / first payload
    byte), L - 1 (the tag's last byte), L // 2 and L - 5 (with a 4-byte tag: the
    byte before it in SRTP, the index word in SRTCP), clamped into the packet."""
    out = {}
    for i in range(0, len(lengths), 3):
        L = int(lengths[i])
        if L <= 0:
            continue
        at = (1, 5, 12, L - 1, L // 2, L - 5)[(i // 3) % 6]
        out[i] = min(max(at, 0), L - 1)
    return out


def tamper_seg(seg, off, lengths):
    """A copy of seg with bit 4 of one byte flipped in every third packet."""
    seg = seg.copy()
    for i, at in tamper_positions(lengths).items():
        seg[int(off[i]) + at] ^= 0x10
    return seg


def tamper(b: synth.Bundle, lengths) -> synth.Bundle:
    """b (protected: `lengths` are its packets' lengths now) with one fault in
    every third packet; see tamper_positions."""
    out = b.copy()
    out.length = np.asarray(lengths, np.uint32).copy()
    out.seg = tamper_seg(b.seg, b.off, lengths)
    return out


def slices(b: synth.Bundle, size: int):
    """b cut into bundles of up to `size` consecutive packets; each shares b's
    bytes (regions are contiguous, so a slice of the segment holds them all)."""
    out = []
    for a in range(0, b.n, size):
        z = min(a + size, b.n)
        lo = int(b.off[a])
        hi = int(b.off[z - 1]) + int(b.cap[z - 1])
        out.append(synth.Bundle(b.seg[lo:hi].copy(), (b.off[a:z] - np.uint32(lo)).astype(np.uint32),
                                b.length[a:z].copy(), b.cap[a:z].copy(), b.flags[a:z].copy(),
                                b.ssrc[a:z].copy(), b.seq[a:z].copy(), {}))
    return out


def spread_ssrcs(b: synth.Bundle, rtcp: bool, ways: int, step: int = 0x100) -> synth.Bundle:
    """A copy of b in which packet i's SSRC is raised by (i % ways) * step: with
    packet i going to transformer i % ways, each transformer gets its own
    ssrc_base."""
    out = b.copy()
    out.ssrc = (b.ssrc + (np.arange(b.n) % ways).astype(np.uint32) * np.uint32(step)).astype(np.uint32)
    _be32(out.seg, out.off.astype(np.int64) + (4 if rtcp else 8), out.ssrc)
    return out
