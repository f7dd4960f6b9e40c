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

} // namespace srtp
