// fanout_job.h -- what one destination entry of a fan-out (srtp_fanout_device /
// _host: m source packets, n entries of (source index, transformer, destination
// region)) gets before the protect chain sees it: skipped, or a copy of its
// source of so many bytes and the source's length.  One plain function that the
// host compiles (srtp_fanout_job, tools/fanout_check.cpp under AddressSanitizer
// + UBSan) and k_fanout compiles as it stands (no HIP type, no pointer): the
// kernel copies exactly copy_bytes, and no byte count leaves here before it is
// shown to lie inside both regions.  All arithmetic is signed int.
//
// The rules:
//   skipped   src_idx < 0 or >= m; the source's status is not OK (the reference's
//             null element: a packet reverseTransform dropped is never written
//             by the translator); the caller's flags carry SKIP.  Nothing is
//             copied, flags_out = caller's | SKIP, len_out = 0: the entry ends
//             SRTP_STATUS_SKIPPED.  by_source tells the first two reasons from
//             the third (srtp_fanout_stats.skipped).
//   otherwise len_out = src_len and copy_bytes = min(src_len, src_cap, dst_cap)
//             rounded up to 16: never past dst_cap rounded up to 16 nor past
//             src_cap rounded up to 16, which is what a region owns
//             (srtp_transform_device).  A source longer than dst_cap keeps its
//             length, and the parse answers DROP_INVALID (len > cap,
//             RawPacket.isInvalid) as for a host-made copy; a region too small
//             for the trailer ends ERR_CAPACITY there.  A length or capacity
//             that is negative as an int (above 2^31 as the uint32 it came from)
//             copies nothing; one above 65535 (no region is larger: the
//             kernels' 16-bit length fields) counts as 65535.
// Fan-out decides nothing else about a packet: the rest is the protect chain's.
//
// Per-destination rewriting (srtp_fanout_device_rw / _host_rw): entry j may
// carry a 16-byte record (mask, ssrc, timestamp, seq, pt; host byte order) that
// gives its copy the target values of the peer's send chain -- what the
// reference's ExtendedSequenceNumberInterval.rewriteRTP does through four
// RawPacket setters in front of the stream's SRTP transformer:
//   SSRC       setSSRC:           bytes 8..11 = ssrc, big-endian
//   SEQ        setSequenceNumber: bytes 2..3  = seq, big-endian
//   TIMESTAMP  setTimestamp:      bytes 4..7  = timestamp, big-endian
//   PT         setPayloadType:    byte 1 = (byte 1 & 0x80) | (pt & 0x7F)
// Two more plain functions, compiled alike by the host (srtp_fanout_rewrite_job,
// tools/fanout_rewrite_check.cpp) and by k_fanout_rw:
//   fanout_rewrite_applies  exactly when the entry is not skipped, mask & 0xF
//             is non-zero and c = min(src_len, src_cap, dst_cap), before the
//             rounding, is at least 12.  Then the first 16-byte piece of the
//             copy holds the whole fixed header, so the patch touches no byte
//             the copy did not write.  A copy of fewer than 12 bytes is left as
//             it is (the entry ends DROP_INVALID by the rules above anyway).
//   fanout_rewrite_words    the three little-endian 32-bit words of header
//             bytes 0..11 as loaded, returned patched.
// Bits of mask above 0xF and `reserved` are ignored here.  The rule knows
// nothing about the transformer's kind: it writes the bytes the four setters
// write, as RawPacket does.  For an SRTCP transformer only mask 0 makes sense
// (bytes 4..7 are its SSRC); that is the caller's responsibility.
//
// Abs-send-time (srtp_fanout_device_ast / _host_ast): entry j may also carry an
// 8-byte record (value, id, on) for the third engine of the peer's send chain,
// AbsSendTimeEngine (AbsSendTimeEngine.java:46-152), which overwrites the three
// data bytes of the copy's abs-send-time header-extension element.  Where those
// bytes lie is found by a walk over the packet's own bytes, so the rule is
// templated on a byte reader (rd(i): byte i of the packet, 0..255); no pointer
// enters it.  Compiled alike by the host (srtp_fanout_ast_job,
// tools/fanout_ast_check.cpp) and by k_fanout_ast:
//   fanout_ast_wanted  c = min(src_len, src_cap, dst_cap), clamped as above,
//             when the entry is not skipped, the record is on (on != 0), its id
//             is at most 15 (the reference compares an int with a nibble: a
//             larger one never matches) and c >= 12; else 0.  Asked before any
//             byte is read: 0 means no walk.
//   fanout_ast_find    the offset of the first stamped byte, or -1: the
//             reference's transform / replaceAbsSendTime over a buffer that
//             ends with the c copied bytes (buf.length = c), Java's integer
//             semantics included.  (b[0] >> 6) == 2 and b[0] & 0x10, then
//               p = 12 + 4 * (b[0] & 15) + 2; only if p + 1 < c:
//               lw = sbyte(b[p]) << 8 | sbyte(b[p + 1]); nbytes = 4 * (1 + lw)
//               p += 2; while p < c and inner < nbytes: the element b[p]; the
//               first whose id matches ends the walk, stamped at p + 1 .. p + 3
//               if its len is 2 and p + 3 < c; else inner, p += len + 2.
//             The reference's quirks are kept: a length byte >= 0x80 makes lw
//             negative (nothing is walked); the "defined by profile" word is
//             not looked at; nbytes counts four bytes too many, and a match
//             there is stamped, into the payload; a padding byte advances by
//             2, and with id 0 is a match of len 0; the first match decides.
//             rd is asked only for 0 <= i < c, and p + 3 < c: every stamped
//             byte is one the copy wrote.
//   fanout_ast_piece   the 16-byte piece q of the copy (four little-endian
//             words) with whichever of the bytes at .. at + 2 lie in it
//             replaced by fanout_ast_bytes(value) = value >> 16, >> 8, >> 0
//             (the top 8 bits of value are ignored), every other byte
//             untouched: a stamp that straddles two pieces is two calls.
//             Selects only, no branch.
// The four setters touch bytes 1..11 and the walk reads b[0] of the fixed header
// only, which no setter writes; the stamp lies at byte 17 or later.  So the two
// rules are independent of the order they are applied in.
//
// Payload patches (srtp_fanout_device_pay / _host_pay): entry j may also carry
// an 8-byte record of two patches (at0, b0[2], at1, b1[2]), the last things
// ExtendedSequenceNumberInterval.rewriteRTP writes with a value of the peer's:
//   RTX  rewriteRTX (:261-284): setOriginalSequenceNumber = writeShort(
//        getHeaderLength(), sn) (RawPacket.java:1018-1022, 1334-1337), two
//        bytes, big-endian, at the start of the payload
//   FEC  rewriteFEC (:346-386), plain or as a RED packet's block (rewriteRED,
//        :307-333): the SN base of the FEC header, buf[off + 2], buf[off + 3]
// Which offset and which bytes is the host's business (getHeaderLength, the RED
// block walk, the peer's numbers): the rule gets offsets and bytes and knows no
// protocol.  Plain functions again, compiled alike by the host
// (srtp_fanout_pay_job, tools/fanout_pay_check.cpp) and by k_fanout_pay:
//   fanout_pay_bound   c = min(src_len, src_cap, dst_cap), clamped as above,
//             when the entry is not skipped and copy_bytes >= c; else 0.
//   fanout_pay_on      a patch is on exactly when at >= 12 and c > at.  A patch
//             below byte 12 is refused whole (at = 0 is the record's "off"):
//             those bytes are the setters', so patches and setters are disjoint
//             and apply in either order.
//   which bytes        byte i of {at, at + 1} of a patch that is on is written
//             iff i < c -- per byte, as the reference's two writeByte calls:
//             with at == c - 1 the first byte is written and the second is
//             not.  No byte is written that the copy did not write.
//   fanout_pay_piece   the 16-byte piece q of the copy (four little-endian
//             words) with whichever of those bytes lie in it replaced by v0
//             (at) and v1 (at + 1), every other byte untouched: a patch that
//             straddles two pieces is two calls.  Selects only, no branch.
//   the order          patch 0, then patch 1 (where they overlap patch 1 wins),
//             then the abs-send-time stamp (where they overlap the stamp wins):
//             the reference's chain, ssrcRewritingEngine (MediaStreamImpl.java:
//             998) in front of absSendTimeEngine (:1018-1020).  The stamp can
//             reach payload bytes through its kept quirk: a match in the four
//             bytes past the extension is stamped into the first payload bytes,
//             where the OSN lies.  The reference's walk reads the copy the
//             rewriting engine has already written, and the same quirk lets it
//             read the first payload bytes as an element: so the walk reads
//             every byte through fanout_pay_byte (the byte as both patches
//             leave it), not the source's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRTP_FANOUT_HD __host__ __device__
#else
#define SRTP_FANOUT_HD
#endif

namespace srtp {

constexpr uint32_t kFanFlagSkip = 0x80000000u; // SRTP_PKT_FLAG_SKIP (this header stands alone)
constexpr int kFanStatusOk = 0;                // SRTP_STATUS_OK
constexpr int kFanMaxRegion = 65535;           // validate_regions: cap <= 65535
constexpr uint32_t kFanRewriteSsrc = 0x1u, kFanRewriteSeq = 0x2u, kFanRewriteTimestamp = 0x4u,
                   kFanRewritePt = 0x8u, kFanRewriteAll = 0xFu; // SRTP_REWRITE_*
constexpr int kFanHeaderBytes = 12;            // the fixed RTP header (RawPacket.FIXED_HEADER_SIZE)

struct FanoutJob {
    int32_t copy_bytes; // a multiple of 16; 0: nothing to copy
    int32_t len_out;    // the entry's length (the source's, as the uint32 it was)
    uint32_t flags_out; // the entry's flags word
    int32_t by_source;  // 1: skipped for its index or its source's status
};

SRTP_FANOUT_HD inline int fanout_clamp(int v) { return v < 0 ? 0 : v > kFanMaxRegion ? kFanMaxRegion : v; }

// src_len, src_cap, src_status: the source's, read only when src_idx is in
// range (any value otherwise); src_status 0 where the caller gave no statuses.
SRTP_FANOUT_HD inline FanoutJob fanout_job(int src_idx, int m, int src_len, int src_cap, int src_status,
                                           int dst_cap, uint32_t caller_flags) {
    FanoutJob j;
    j.copy_bytes = 0;
    j.len_out = 0;
    j.flags_out = caller_flags | kFanFlagSkip;
    j.by_source = 0;
    if (src_idx < 0 || src_idx >= m || src_status != kFanStatusOk) {
        j.by_source = 1;
        return j;
    }
    if (caller_flags & kFanFlagSkip) return j;
    j.flags_out = caller_flags;
    j.len_out = src_len;
    if (src_len < 0 || src_cap < 0 || dst_cap < 0) return j; // no such region: the parse refuses the entry
    const int sc = fanout_clamp(src_cap), dc = fanout_clamp(dst_cap);
    int c = fanout_clamp(src_len);
    if (c > sc) c = sc;
    if (c > dc) c = dc;
    const int copy = (c + 15) & ~15; // c <= 65535: at most 65536
    // The proof, once more, on what is about to be handed out.  It cannot fail
    // by the lines above; should an edit break one, nothing is copied.
    const bool ok = copy >= 0 && (copy & 15) == 0 && copy <= ((sc + 15) & ~15) && copy <= ((dc + 15) & ~15);
    j.copy_bytes = ok ? copy : 0;
    return j;
}

// `j` is fanout_job's answer for the same src_len, src_cap and dst_cap.
SRTP_FANOUT_HD inline bool fanout_rewrite_applies(const FanoutJob &j, int src_len, int src_cap, int dst_cap,
                                                  uint32_t mask) {
    if ((j.flags_out & kFanFlagSkip) || (mask & kFanRewriteAll) == 0u) return false;
    if (src_len < 0 || src_cap < 0 || dst_cap < 0) return false;
    int c = fanout_clamp(src_len);
    const int sc = fanout_clamp(src_cap), dc = fanout_clamp(dst_cap);
    if (c > sc) c = sc;
    if (c > dc) c = dc;
    return c >= kFanHeaderBytes && j.copy_bytes >= 16; // the header lies inside the first piece copied
}

struct FanoutWords {
    uint32_t w0, w1, w2; // header bytes 0..3, 4..7, 8..11, loaded little-endian
};

SRTP_FANOUT_HD inline uint32_t fanout_be32(uint32_t v) {
    return (v >> 24) | ((v >> 8) & 0x0000FF00u) | ((v << 8) & 0x00FF0000u) | (v << 24);
}

SRTP_FANOUT_HD inline FanoutWords fanout_rewrite_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t mask,
                                                       uint32_t ssrc, uint32_t timestamp, uint32_t seq,
                                                       uint32_t pt) {
    FanoutWords w;
    w.w0 = w0;
    w.w1 = w1;
    w.w2 = w2;
    if (mask & kFanRewritePt) w.w0 = (w.w0 & ~0x00007F00u) | ((pt & 0x7Fu) << 8);
    if (mask & kFanRewriteSeq) w.w0 = (w.w0 & 0x0000FFFFu) | ((seq & 0xFF00u) << 8) | ((seq & 0x00FFu) << 24);
    if (mask & kFanRewriteTimestamp) w.w1 = fanout_be32(timestamp);
    if (mask & kFanRewriteSsrc) w.w2 = fanout_be32(ssrc);
    return w;
}

// ---- abs-send-time (srtp_fanout_device_ast / _host_ast, k_fanout_ast)

// c = min(src_len, src_cap, dst_cap) clamped as above when entry j's record can stamp at all --
// the entry is not skipped, the record is on, its ID fits a nibble and the fixed header was
// copied -- else 0.  Asked before any byte of the packet is read: 0 means no walk.
SRTP_FANOUT_HD inline int fanout_ast_wanted(const FanoutJob &j, int src_len, int src_cap, int dst_cap, uint32_t on,
                                            uint32_t ext_id) {
    if ((j.flags_out & kFanFlagSkip) || on == 0u || ext_id > 15u) return 0;
    if (src_len < 0 || src_cap < 0 || dst_cap < 0) return 0;
    int c = fanout_clamp(src_len);
    const int sc = fanout_clamp(src_cap), dc = fanout_clamp(dst_cap);
    if (c > sc) c = sc;
    if (c > dc) c = dc;
    return c >= kFanHeaderBytes && j.copy_bytes >= c ? c : 0; // every byte below c is one the copy writes
}

SRTP_FANOUT_HD inline int fanout_sbyte(int b) { return b >= 128 ? b - 256 : b; } // a Java byte

// The offset of the first of the three bytes AbsSendTimeEngine would overwrite, or -1.  rd(i)
// is byte i of the packet and is asked only for 0 <= i < c.
template <class Rd>
SRTP_FANOUT_HD inline int fanout_ast_find(Rd rd, const FanoutJob &j, int src_len, int src_cap, int dst_cap,
                                          uint32_t on, uint32_t ext_id) {
    const int B = fanout_ast_wanted(j, src_len, src_cap, dst_cap, on, ext_id);
    if (B == 0) return -1;
    const int b0 = rd(0);
    if ((b0 >> 6) != 2 || (b0 & 0x10) == 0) return -1; // getVersion() == 2 && getExtensionBit()
    int p = kFanHeaderBytes + 4 * (b0 & 15) + 2;       // behind the CSRCs and "defined by profile"
    if (!(p + 1 < B)) return -1;
    const int lw = (fanout_sbyte(rd(p)) * 256) | fanout_sbyte(rd(p + 1)); // buf[p] << 8 | buf[p + 1], signed bytes
    const int nbytes = 4 * (1 + lw);
    p += 2;
    int inner = 0;
    while (p < B && inner < nbytes) {
        const int e = rd(p);
        const int len = e & 15;
        if ((e >> 4) == (int)ext_id) return len == 2 && p + 3 < B ? p + 1 : -1;
        inner += len + 2;
        p += len + 2;
    }
    return -1;
}

struct FanoutBytes {
    uint32_t b0, b1, b2; // in the packet's order
};
SRTP_FANOUT_HD inline FanoutBytes fanout_ast_bytes(uint32_t value) {
    FanoutBytes b;
    b.b0 = (value >> 16) & 0xFFu;
    b.b1 = (value >> 8) & 0xFFu;
    b.b2 = value & 0xFFu;
    return b;
}

struct FanoutPiece {
    uint32_t w0, w1, w2, w3; // bytes 16q .. 16q + 15 of the copy, loaded little-endian
};

// One word of a piece: `s` is where the stamp starts relative to the word's first byte.
// Without a branch (selects only: in the kernel this sits between a trip's loads and its stores):
// for s in -2 .. 3 the three bytes, two bytes in front of the word, are moved s + 2 bytes up and
// the word's four are kept.
SRTP_FANOUT_HD inline uint32_t fanout_ast_word(uint32_t w, int s, uint32_t v) {
    const bool in = s >= -2 && s <= 3;
    const int up = in ? 8 * (s + 2) : 0; // 0 .. 40
    const uint32_t m = (uint32_t)(((uint64_t)0x00FFFFFFu << up) >> 16);
    const uint32_t x = (uint32_t)(((uint64_t)v << up) >> 16);
    return in ? (w & ~m) | x : w;
}

// Piece q with whichever of the bytes at .. at + 2 lie in it replaced (at >= 0).
SRTP_FANOUT_HD inline FanoutPiece fanout_ast_piece(const FanoutPiece &piece, int q, int at, uint32_t value) {
    const FanoutBytes b = fanout_ast_bytes(value);
    const uint32_t v = b.b0 | (b.b1 << 8) | (b.b2 << 16); // the three bytes as memory holds them
    const int s = at - 16 * q;
    FanoutPiece o;
    o.w0 = fanout_ast_word(piece.w0, s, v);
    o.w1 = fanout_ast_word(piece.w1, s - 4, v);
    o.w2 = fanout_ast_word(piece.w2, s - 8, v);
    o.w3 = fanout_ast_word(piece.w3, s - 12, v);
    return o;
}

// ---- payload patches (srtp_fanout_device_pay / _host_pay, k_fanout_pay)

// c = min(src_len, src_cap, dst_cap) clamped as above when entry j can be patched at all -- it is
// not skipped and every byte below c is one the copy writes -- else 0.
SRTP_FANOUT_HD inline int fanout_pay_bound(const FanoutJob &j, int src_len, int src_cap, int dst_cap) {
    if (j.flags_out & kFanFlagSkip) return 0;
    if (src_len < 0 || src_cap < 0 || dst_cap < 0) return 0;
    int c = fanout_clamp(src_len);
    const int sc = fanout_clamp(src_cap), dc = fanout_clamp(dst_cap);
    if (c > sc) c = sc;
    if (c > dc) c = dc;
    return j.copy_bytes >= c ? c : 0;
}

// A patch at `at` (0 .. 65535, the record's uint16) of an entry whose bound is c.
SRTP_FANOUT_HD inline bool fanout_pay_on(int at, int c) { return at >= kFanHeaderBytes && c > at; }

// One word of a piece: `s` is where the patch starts relative to the word's first byte; w0 / w1:
// whether the patch's first / second byte is written at all.  Selects only, as fanout_ast_word.
SRTP_FANOUT_HD inline uint32_t fanout_pay_word(uint32_t w, int s, uint32_t v0, uint32_t v1, bool w0, bool w1) {
    const bool in0 = w0 && s >= 0 && s <= 3, in1 = w1 && s >= -1 && s <= 2;
    const int up0 = in0 ? 8 * s : 0, up1 = in1 ? 8 * (s + 1) : 0; // 0 .. 24
    const uint32_t m = (in0 ? 0xFFu << up0 : 0u) | (in1 ? 0xFFu << up1 : 0u);
    const uint32_t x = (in0 ? (v0 & 0xFFu) << up0 : 0u) | (in1 ? (v1 & 0xFFu) << up1 : 0u);
    return (w & ~m) | x;
}

// Piece q with whichever of the bytes at (v0), at + 1 (v1) are written and lie in it replaced:
// nothing when the patch is off, the first byte only when at == c - 1.
SRTP_FANOUT_HD inline FanoutPiece fanout_pay_piece(const FanoutPiece &piece, int q, int at, uint32_t v0, uint32_t v1,
                                                   int c) {
    const bool w0 = fanout_pay_on(at, c), w1 = w0 && at + 1 < c;
    const int s = at - 16 * q;
    FanoutPiece o;
    o.w0 = fanout_pay_word(piece.w0, s, v0, v1, w0, w1);
    o.w1 = fanout_pay_word(piece.w1, s - 4, v0, v1, w0, w1);
    o.w2 = fanout_pay_word(piece.w2, s - 8, v0, v1, w0, w1);
    o.w3 = fanout_pay_word(piece.w3, s - 12, v0, v1, w0, w1);
    return o;
}

// Byte i of the copy (b as the source holds it) behind one patch: what fanout_pay_piece leaves
// there.  The abs-send-time walk of a patched entry reads through this, patch 0 then patch 1.
SRTP_FANOUT_HD inline int fanout_pay_byte(int b, int i, int at, uint32_t v0, uint32_t v1, int c) {
    const bool w0 = fanout_pay_on(at, c), w1 = w0 && at + 1 < c;
    return w0 && i == at ? (int)(v0 & 0xFFu) : w1 && i == at + 1 ? (int)(v1 & 0xFFu) : b;
}

} // namespace srtp
