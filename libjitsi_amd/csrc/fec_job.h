// fec_job.h -- what an FEC entry of a fan-out (srtp_fanout_device_fec /
// _host_fec) becomes: the ulpfec packet (RFC 5109, one level, short mask) over
// up to 16 member entries of the same call, as they stand in the destination
// segment behind all their records and in front of the protect chain.  Plain
// functions that the host compiles (srtp_fanout_fec_job, tools/
// fanout_fec_check.cpp under AddressSanitizer + UBSan) and k_fanout_fec compiles
// as they stand: no HIP type and no pointer.  The members' bytes come in as
// aligned little-endian words that the caller loaded; which piece and which
// word to load is said here, and every byte at or past a member's len is masked
// off before it is used, so a caller may load whatever lies between len and len
// rounded up to 16 and nothing past that.  All arithmetic is signed int or
// uint32.
//
// The reference, restated: FECSender.FECPacket (transform/fec/FECSender.java),
// addMedia (:319-380) on the members in list order, then finish (:387-412);
// for mode 2 REDTransformEngine.transform (transform/REDTransformEngine.java:
// 151-182) on the finished packet, whose header length is 12.
//   addMedia  mediaPayloadLen = len - 12 ("payload" is everything behind the
//             fixed 12 bytes, CSRCs and extension included).  The first member
//             is copied, every later one XORed: bytes 12..19 ^= member bytes
//             0..7, bytes 20..21 ^= mediaPayloadLen (big-endian), bytes 26.. ^=
//             member bytes 12 .. len - 1.  The buffer starts as zeros and is
//             grown with zeros, so copy and XOR are one rule and a shorter
//             member contributes zeros past its length.  base = the first
//             member's sequence number, lastAddedSeq / lastAddedTS the last
//             one's, protectionLength = max(mediaPayloadLen), numPackets++.
//   finish    byte 0 = 0x80; setPayloadType(pt): byte 1 = (0 & 0x80) | (pt &
//             0x7F); setSequenceNumber(lastAddedSeq + 1): two bytes, big-endian,
//             65536 written as 0; setSSRC; setTimestamp(lastAddedTS); bytes
//             14..15 = base (over the XOR of the members' sequence numbers);
//             bytes 22..23 = protectionLength; bytes 24..25 = ((1 << n) - 1) <<
//             (16 - n): the members are taken to be consecutive; length = 26 +
//             protectionLength.  Byte 12 stays the plain XOR of the members'
//             first bytes: with an odd count of version-2 members the E bit
//             comes out set.  Kept.
//   the wrap  newBuf[12] = getPayloadType() = pt & 0x7F, bytes 12.. move up by
//             one, byte 1 = red_pt, length + 1.
//
//   fec_record_ok     the entry's own record and source index: mode 1 or 2,
//             count 1..16 (fecRate "should be in [0, 16]",
//             FECTransformEngine.java:236), first + count <= n_members, pt <=
//             127, red_pt <= 127 with mode 2, src_idx == -1 (an FEC entry has
//             no source).
//   fec_member_index_ok, fec_member_ok, fec_member_v2   a member is an entry of
//             the call (0 <= index < n) that does not carry SKIP after the
//             expansion, whose own record is off (no FEC over FEC: members are
//             read-only inputs of the launch), with 12 <= len <= cap <= 65535,
//             and version 2 (FECSender.transform's test, :103).  Asked in this
//             order: the index before anything of the member is read, the
//             lengths before its first byte is.
//   FecHead, fec_head_word   the 26 (27) header bytes, as words 0..7 of the
//             packet, from the scalars a wave reduces: the XOR of the members'
//             first two words, of len - 12, the maximum of len - 12, the first
//             member's word 0 and the last member's words 0 and 1.
//   fec_src_piece, fec_src_word, fec_accumulate, fec_piece   a 16-byte piece q
//             of the packet.  Output byte d is member byte d - 14 (plain) or d -
//             15 (wrapped), and regions start 16-byte aligned, so piece q needs
//             of each member its aligned piece q - 1 and its aligned word 4 q:
//             a window of 20 bytes from member byte 16 (q - 1) on, funnelled
//             down by 2 bytes or 1.  XOR, the mask and the funnel are linear,
//             so the members' masked windows are XORed first (fec_accumulate)
//             and funnelled once (fec_piece), which also ORs the header in:
//             window bytes below member byte 12 are masked too, so header and
//             payload never overlap.  Where the window's piece or word does not
//             lie below len, piece 0 or word 0 is named instead (len >= 12:
//             they exist) and the mask discards it: every load is unconditional
//             and none goes at or past len rounded up to 16.
#pragma once
#include "fanout_job.h"

namespace srtp {

constexpr int kFecOff = 0, kFecPlain = 1, kFecRed = 2;          // srtp_fanout_fec.mode
constexpr int kFecNone = 0, kFecMade = 1, kFecRefused = -1;     // fec_out
constexpr int kFecMaxMembers = 16, kFecHeaderBytes = 26;        // RTP_HDR_LEN + FEC_HDR_LEN

SRTP_FANOUT_HD inline bool fec_record_ok(uint32_t first, uint32_t count, uint32_t pt, uint32_t red_pt, uint32_t mode,
                                         uint32_t n_members, int own_src_idx) {
    if (mode != (uint32_t)kFecPlain && mode != (uint32_t)kFecRed) return false;
    if (count < 1u || count > (uint32_t)kFecMaxMembers) return false;
    if (first > n_members || count > n_members - first) return false;
    if (pt > 127u || (mode == (uint32_t)kFecRed && red_pt > 127u)) return false;
    return own_src_idx == -1;
}

SRTP_FANOUT_HD inline bool fec_member_index_ok(int mi, int n) { return mi >= 0 && mi < n; }
// flags: the member's flags word after the expansion; mode: its own record's
SRTP_FANOUT_HD inline bool fec_member_ok(uint32_t flags, uint32_t mode, int len, int cap) {
    if ((flags & kFanFlagSkip) || mode != (uint32_t)kFecOff) return false;
    return len >= kFanHeaderBytes && cap >= 0 && cap <= kFanMaxRegion && len <= cap;
}
// w0: the member's bytes 0..3, little-endian
SRTP_FANOUT_HD inline bool fec_member_v2(uint32_t w0) { return ((w0 >> 6) & 3u) == 2u; }

struct FecHead {
    uint32_t x0, x1;           // the XOR of the members' words 0 and 1
    uint32_t first_w0;         // the first member's word 0 (its sequence number: SN base)
    uint32_t last_w0, last_w1; // the last member's words 0 and 1 (its sequence number and timestamp)
    int len_xor, plen;         // XOR and maximum of len - 12
    int count, mode;
    uint32_t ssrc, pt, red_pt;
};

SRTP_FANOUT_HD inline uint32_t fec_be16(uint32_t v) { return ((v >> 8) & 0xFFu) | ((v & 0xFFu) << 8); }
SRTP_FANOUT_HD inline int fec_header_bytes(int mode) { return kFecHeaderBytes + (mode == kFecRed ? 1 : 0); }
SRTP_FANOUT_HD inline int fec_len_out(const FecHead &h) { return fec_header_bytes(h.mode) + h.plen; }
// how far up the window is funnelled down: output byte d is member byte d - 16 + this
SRTP_FANOUT_HD inline int fec_shift(int mode) { return mode == kFecRed ? 1 : 2; }

// Word k (0..7) of the plain packet's header: bytes 4 k .. 4 k + 3, zero from byte 26 on.
SRTP_FANOUT_HD inline uint32_t fec_plain_word(int k, const FecHead &h) {
    const uint32_t last_seq = (((h.last_w0 >> 16) & 0xFFu) << 8) | (h.last_w0 >> 24);
    const uint32_t seq = (last_seq + 1u) & 0xFFFFu;
    const uint32_t mask = (((1u << h.count) - 1u) << (16 - h.count)) & 0xFFFFu;
    return k == 0   ? 0x80u | ((h.pt & 0x7Fu) << 8) | (fec_be16(seq) << 16)
           : k == 1 ? h.last_w1
           : k == 2 ? fanout_be32(h.ssrc)
           : k == 3 ? (h.x0 & 0x0000FFFFu) | (h.first_w0 & 0xFFFF0000u)
           : k == 4 ? h.x1
           : k == 5 ? fec_be16((uint32_t)h.len_xor) | (fec_be16((uint32_t)h.plen) << 16)
           : k == 6 ? fec_be16(mask)
                    : 0u;
}
// Word k (0..7) of the packet's header as it is sent: the plain one, or wrapped in RED.
SRTP_FANOUT_HD inline uint32_t fec_head_word(int k, const FecHead &h) {
    const uint32_t p = fec_plain_word(k, h);
    if (h.mode != kFecRed) return p;
    if (k == 0) return (p & ~0x0000FF00u) | ((h.red_pt & 0x7Fu) << 8);
    if (k < 3) return p;
    const uint32_t below = k == 3 ? (h.pt & 0x7Fu) : fec_plain_word(k - 1, h) >> 24;
    return (p << 8) | below;
}

// Which aligned piece and word of a member feed output piece q (len >= 12).
SRTP_FANOUT_HD inline int fec_src_piece(int q, int len) { return q >= 1 && 16 * (q - 1) < len ? q - 1 : 0; }
SRTP_FANOUT_HD inline int fec_src_word(int q, int len) { return q >= 0 && 16 * q < len ? 4 * q : 0; }

// The bytes of a word at member byte `base` that belong to the payload: base + b in [12, len).
SRTP_FANOUT_HD inline uint32_t fec_mask(int base, int len) {
    const int r = len - base;
    return base < kFanHeaderBytes || r <= 0 ? 0u : r >= 4 ? 0xFFFFFFFFu : (1u << (8 * r)) - 1u;
}

struct FecWindow {
    uint32_t w0, w1, w2, w3, w4; // member bytes 16 (q - 1) .. 16 q + 3, masked, XORed over the members
};

// P: the member's piece fec_src_piece(q, len); W: its word fec_src_word(q, len).  len 0: nothing.
SRTP_FANOUT_HD inline void fec_accumulate(FecWindow &a, const FanoutPiece &P, uint32_t W, int q, int len) {
    const int base = 16 * (q - 1);
    a.w0 ^= P.w0 & fec_mask(base, len);
    a.w1 ^= P.w1 & fec_mask(base + 4, len);
    a.w2 ^= P.w2 & fec_mask(base + 8, len);
    a.w3 ^= P.w3 & fec_mask(base + 12, len);
    a.w4 ^= W & fec_mask(base + 16, len);
}

SRTP_FANOUT_HD inline uint32_t fec_funnel(uint32_t lo, uint32_t hi, int s) {
    return (lo >> (8 * s)) | (hi << (32 - 8 * s)); // s is 1 or 2
}

// Piece q of the packet from the XORed windows and the header.
SRTP_FANOUT_HD inline FanoutPiece fec_piece(const FecWindow &a, int q, const FecHead &h) {
    const int s = fec_shift(h.mode);
    FanoutPiece o;
    o.w0 = fec_funnel(a.w0, a.w1, s);
    o.w1 = fec_funnel(a.w1, a.w2, s);
    o.w2 = fec_funnel(a.w2, a.w3, s);
    o.w3 = fec_funnel(a.w3, a.w4, s);
    if (q < 2) { // the header's words lie where every window byte was masked off
        o.w0 |= fec_head_word(4 * q, h);
        o.w1 |= fec_head_word(4 * q + 1, h);
        o.w2 |= fec_head_word(4 * q + 2, h);
        o.w3 |= fec_head_word(4 * q + 3, h);
    }
    return o;
}

// How many bytes of the packet are stored: below min(len_out, cap) rounded up to 16, which a region owns.
SRTP_FANOUT_HD inline int fec_store_bytes(int len_out, int dst_cap) {
    if (len_out < 0 || dst_cap < 0) return 0;
    const int dc = fanout_clamp(dst_cap);
    const int c = len_out < dc ? len_out : dc;
    const int store = (c + 15) & ~15;
    return store <= ((dc + 15) & ~15) ? store : 0;
}

} // namespace srtp
