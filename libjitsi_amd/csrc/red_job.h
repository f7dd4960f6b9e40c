// red_job.h -- what one destination entry of a fan-out gets from the RED
// (RFC 2198) step of the peer's send chain (srtp_fanout_device_red / _host_red),
// in front of every other per-destination record: nothing, the one-byte RED
// header of a single-block packet taken out (the peer did not negotiate RED),
// the header put in (the peer did and the source sent none), or the entry
// dropped where the reference throws.  Plain functions that the host compiles
// (srtp_fanout_red_job, tools/fanout_red_check.cpp under AddressSanitizer +
// UBSan) and k_fanout_red compiles as they stand: no HIP type and no pointer;
// the packet's bytes come through a byte reader rd(i), byte i of the packet
// (0..255), asked only for 0 <= i < c.  All arithmetic is signed int, and a byte
// is Java's signed byte wherever the reference reads it as one.  The convention
// is fanout_ast_find's: the reference's buffer ends with the c copied bytes
// (buf.length = c, offset 0, length c).
//
// The reference, restated:
//   strip  REDFilterTransformEngine.transform (transform/
//          REDFilterTransformEngine.java:95-145), a SinglePacketTransformer
//          behind RTPPacketPredicate (AbstractRTPPacketPredicate.test, :53-97),
//          over REDBlockIterator.getPrimaryBlock (codec/REDBlockIterator.java:
//          118-166), isMultiBlock (:178-193), initialize (:276-317) and next
//          (:217-265)
//   wrap   REDTransformEngine.transform (transform/REDTransformEngine.java:
//          151-182; in the chain at MediaStreamImpl.java:993-996)
//   both   RawPacket.getHeaderLength (RawPacket.java:602-614) over
//          getExtensionLength (:544-556), getPayloadType (:760-763) and
//          setPayloadType (:1240-1247)
//
//   red_wanted(job, src_len, src_cap, dst_cap, mode, red_pt, reserved) -> c or
//          0.  The step is asked for only when the entry is not skipped, mode is
//          SRTP_RED_STRIP or SRTP_RED_WRAP, red_pt <= 127 (the reference's -1,
//          "disabled", is mode 0), reserved is 0, c = min(src_len, src_cap,
//          dst_cap) clamped as fanout_job clamps is at least 12 and c ==
//          clamp(src_len): the whole packet is there.  Asked before any byte is
//          read: 0 means no byte is, the result is 0 and the entry is the _pay
//          call's.
//   red_header_length(rd, c, &oob) -> h = getHeaderLength():
//            h = 12 + 4 * (b[0] & 15); if b[0] & 0x10:
//              p = h + 2; h += 4 + ((sbyte(b[p]) << 8) | (b[p + 1] & 0xFF)) * 4
//          the first byte signed, the second not (RawPacket.java:555).  h is a
//          multiple of 4, in -131056 .. 131144.  A read at p or p + 1 >= c is the
//          reference's ArrayIndexOutOfBounds: oob is set and nothing is read.
//   red_rule(rd, c, mode, red_pt) -> RedPlan.
//     strip, in the reference's order:
//       1. (b0 >> 6) != 2: 0 (the predicate's getVersion() == 2, :62)
//       2. b1 & 0xFF in 200..211: 0 (the predicate's RTCP test, :66-75, kept
//          with its quirk: marker set with PT 72..83 is never stripped)
//       3. (b1 & 0x7F) != red_pt: 0 (REDFilterTransformEngine.java:119-123)
//       4. h = getHeaderLength() (getPayloadOffset, :126); out of bounds: -1
//       5. h < 0 or h > c: 0.  isMultiBlock answers false (offset < 0 ||
//          buffer.length <= offset, REDBlockIterator.java:186-190) and
//          getPrimaryBlock's guards (offset < 0 || length < 0, :145-152; length
//          is c - h) return null: "no primary block", the packet goes on
//          unchanged (REDFilterTransformEngine.java:128-132)
//       6. h == c: -1.  isMultiBlock is false again, the guards pass (length 0,
//          c < c + 0 is false) and buffer[offset] (:154) throws
//       7. b = rd(h)
//       8. b & 0x80: -1.  At this revision a multi-block packet always throws.
//          initialize walks `while (buffer[off] & 0x80) off += 4` (:294-298)
//          either off the buffer (ArrayIndexOutOfBounds) or to a header with
//          F = 0, with cntRemainingBlocks >= 1 (b itself had F = 1).  Every
//          next() of getPrimaryBlock's loop (:131-134) finds buffer.length >
//          offNextBlockHeader (initialize read that far), so none but a middle
//          one returns null, and the last one takes the else branch and hands
//          the primary block back as REDBlock(offNextBlockPayload = -1, ..)
//          (:259-264).  transform then calls System.arraycopy(buf, off, buf,
//          -1 - hdrLen, hdrLen) (REDFilterTransformEngine.java:140): a negative
//          destPos throws whatever the length.
//       9. otherwise 1.  pb.getOffset() = h + 1; setPayloadType(b & 0x7F), the
//          header moved one byte up, offset 1, length c - 1: the new packet is
//          bytes 0 .. h - 1 with byte 1 = (b1 & 0x80) | (b & 0x7F), followed by
//          source bytes h + 1 .. c - 1.  (h is 0 or at least 4; with h == 0,
//          b = b0 has bit 7 set under version 2 and step 8 has answered.)
//      10. The quirk blockLen = length - blockOff (:156) subtracts an offset
//          from a length: (c - h) - (h + 1).  Its one use is the guard
//          buffer.length < blockOff + blockLen (:158), which is c < c - h:
//          false for every 0 <= h < c.  transform never reads blockLen.  So the
//          quirk cannot change the outcome.
//     wrap (no predicate and no PT test; outgoingPT == -1 is mode 0):
//       1. (b0 >> 6) != 2: 0 (getVersion() == RTPHeader.VERSION, :158)
//       2. h = getHeaderLength() (:163); out of bounds: -1
//       3. h < 0 or h > c: -1.  System.arraycopy(buf, off, newBuf, 0, hdrLen)
//          (:170) throws
//       4. otherwise 2.  newBuf (c + 1 bytes; buf.length = c < len + 1) gets
//          bytes 0 .. h - 1, then source bytes h .. c - 1 at h + 1 (:171), then
//          newBuf[h] = getPayloadType() = b1 & 0x7F (:172), then
//          setPayloadType(red_pt) (:178) on the new buffer's byte 1: byte 1 =
//          (new byte 1 & 0x80) | red_pt.  New byte 1 is b1 whenever h >= 4; with
//          h == 0 (an extension length of -(4 + CC) words) it is the moved b0,
//          and red_piece writes exactly that.  The new length is c + 1.
//       5. c + 1 > clamp(dst_cap): still 2 and len_out = c + 1; no byte is
//          moved (red_job), and the parse answers DROP_INVALID (len > cap) as
//          it would for a host-made wrapped copy.
//   red_job(job, plan, dst_cap) -> the FanoutJob every later record of the entry
//          is asked with, together with red_src_len / red_src_cap: rewrite, pay
//          and stamp see the packet RED left, in its coordinates, as if the
//          source had held it (ssrcRewritingEngine stands behind RED,
//          MediaStreamImpl.java:998).  A dropped entry (-1) is the reference's
//          lost packet -- the exception leaves SinglePacketTransformer.transform
//          (:194-210) -- : copy_bytes = 0, len_out = 0, flags_out |= SKIP, so it
//          ends SRTP_STATUS_SKIPPED with no context touched.
//   red_piece(A, nb, q, shift, h, ins, pt) -> the 16-byte piece q of the new
//          packet (four little-endian words).  Byte i of it is
//            i < h                 source byte i
//            i == h and shift > 0  ins
//            otherwise             source byte i - shift
//          and then byte 1 = (byte 1 & 0x80) | pt.  h is a multiple of 4, so
//          the choice is per word.  A is source piece q; nb is the one source
//          word beside it that the shift pulls a byte from: word 4 q - 1 for
//          wrap (its top byte), word 4 q + 4 for strip (its low byte).  Selects
//          only, no branch.  red_src_piece / red_src_word say which piece and
//          word to load, clamped into the source's pieces: a clamped load feeds
//          only bytes at or past the new length.
//   red_byte(rd, i, plan)  byte i of the new packet, 0 <= i < len_out, through
//          the source's reader: what red_piece leaves there.  The abs-send-time
//          walk and fanout_pay_byte of a RED entry read through this.
#pragma once
#include "fanout_job.h"

namespace srtp {

constexpr int kRedOff = 0, kRedStrip = 1, kRedWrap = 2;                            // SRTP_RED_*
constexpr int kRedUntouched = 0, kRedStripped = 1, kRedWrapped = 2, kRedDropped = -1; // the result codes

struct RedPlan {
    int result;  // 0, 1, 2 or -1
    int h;       // getHeaderLength() where result is 1 or 2 (0 <= h <= c, a multiple of 4); else 0
    int len_out; // the new packet's length: c - 1, c + 1; c where untouched; 0 where dropped
    int shift;   // -1 strip, +1 wrap, 0 neither
    int ins;     // wrap: the byte put in at h
    int pt;      // the seven bits setPayloadType writes into byte 1
};

// c when the entry's step is asked for, else 0.  `j` is fanout_job's answer for the same lengths.
SRTP_FANOUT_HD inline int red_wanted(const FanoutJob &j, int src_len, int src_cap, int dst_cap, uint32_t mode,
                                     uint32_t red_pt, uint32_t reserved) {
    if (j.flags_out & kFanFlagSkip) return 0;
    if ((mode != (uint32_t)kRedStrip && mode != (uint32_t)kRedWrap) || red_pt > 127u || reserved != 0u) return 0;
    if (src_len < 0 || src_cap < 0 || dst_cap < 0) return 0;
    int c = fanout_clamp(src_len);
    const int sc = fanout_clamp(src_cap), dc = fanout_clamp(dst_cap);
    if (c > sc) c = sc;
    if (c > dc) c = dc;
    if (c < kFanHeaderBytes || c != fanout_clamp(src_len)) return 0;
    return j.copy_bytes >= c ? c : 0; // every byte below c is one the copy loop may load
}

// RawPacket.getHeaderLength over a buffer of c >= 12 bytes.
template <class Rd> SRTP_FANOUT_HD inline int red_header_length(Rd rd, int c, bool &oob) {
    const int b0 = rd(0);
    int h = kFanHeaderBytes + 4 * (b0 & 15);
    oob = false;
    if (b0 & 0x10) {
        const int p = h + 2;
        if (p + 1 >= c) { // buffer[extLenIndex + 1] throws (or buffer[extLenIndex] before it)
            oob = true;
            return 0;
        }
        h += 4 + ((fanout_sbyte(rd(p)) * 256) | rd(p + 1)) * 4;
    }
    return h;
}

SRTP_FANOUT_HD inline RedPlan red_plan_of(int result, int h, int len_out, int shift, int ins, int pt) {
    RedPlan p;
    p.result = result;
    p.h = h;
    p.len_out = len_out;
    p.shift = shift;
    p.ins = ins;
    p.pt = pt;
    return p;
}

// c: red_wanted's answer, not 0.  mode: kRedStrip or kRedWrap.
template <class Rd> SRTP_FANOUT_HD inline RedPlan red_rule(Rd rd, int c, int mode, int red_pt) {
    const RedPlan untouched = red_plan_of(kRedUntouched, 0, c, 0, 0, 0);
    const RedPlan dropped = red_plan_of(kRedDropped, 0, 0, 0, 0, 0);
    const int b0 = rd(0), b1 = rd(1);
    if ((b0 >> 6) != 2) return untouched;
    if (mode == kRedStrip) {
        if (b1 >= 200 && b1 <= 211) return untouched;
        if ((b1 & 0x7F) != red_pt) return untouched;
    }
    bool oob;
    const int h = red_header_length(rd, c, oob);
    if (oob) return dropped;
    if (mode == kRedStrip) {
        if (h < 0 || h > c) return untouched;
        if (h == c) return dropped;
        const int b = rd(h);
        if (b & 0x80) return dropped;
        return red_plan_of(kRedStripped, h, c - 1, -1, 0, b & 0x7F);
    }
    if (h < 0 || h > c) return dropped;
    return red_plan_of(kRedWrapped, h, c + 1, 1, b1 & 0x7F, red_pt);
}

// The job the entry's later records are asked with.
SRTP_FANOUT_HD inline FanoutJob red_job(const FanoutJob &j, const RedPlan &p, int dst_cap) {
    FanoutJob o = j;
    if (p.result == kRedUntouched) return o;
    if (p.result == kRedDropped) {
        o.copy_bytes = 0;
        o.len_out = 0;
        o.flags_out = j.flags_out | kFanFlagSkip;
        return o;
    }
    // A result above 0 implies dst_cap >= c (red_wanted).  Said again here so that fanout_clamp is asked, as by
    // every other caller, only for a value it was shown not to be negative: the compiler folds its `v < 0` from
    // the callers' ranges, and one caller without the test would change the code of all the fan-out kernels.
    const int dc = dst_cap < 0 ? 0 : fanout_clamp(dst_cap);
    const int copy = (p.len_out + 15) & ~15;
    o.len_out = p.len_out;
    // Strip: len_out < c <= dc.  Wrap: only what fits is moved.  The proof, as fanout_job's, on what is handed out.
    const bool ok = p.len_out >= 0 && p.len_out <= dc && copy <= ((dc + 15) & ~15);
    o.copy_bytes = ok ? copy : 0;
    return o;
}
// The source lengths that go with red_job's answer: the new packet's where RED changed it.
SRTP_FANOUT_HD inline int red_src_len(const RedPlan &p, int src_len) { return p.result > 0 ? p.len_out : src_len; }
SRTP_FANOUT_HD inline int red_src_cap(const RedPlan &p, int src_cap) { return p.result > 0 ? kFanMaxRegion : src_cap; }

// Which source piece / word feeds destination piece q (ws > 0: the source's pieces).
SRTP_FANOUT_HD inline int red_src_piece(int q, int ws) { return q < ws ? q : ws - 1; }
SRTP_FANOUT_HD inline int red_src_word(int q, int shift, int ws) {
    const int w = shift > 0 ? 4 * q - 1 : 4 * q + 4;
    return w < 0 ? 0 : w > 4 * ws - 1 ? 4 * ws - 1 : w;
}

SRTP_FANOUT_HD inline uint32_t red_word(uint32_t a, uint32_t s, int base, int shift, int h, uint32_t ins) {
    uint32_t w = base < h ? a : s;
    w = shift > 0 && base == h ? (w & ~0xFFu) | (ins & 0xFFu) : w;
    return w;
}

SRTP_FANOUT_HD inline FanoutPiece red_piece(const FanoutPiece &A, uint32_t nb, int q, int shift, int h, uint32_t ins,
                                            uint32_t pt) {
    const bool up = shift > 0;
    FanoutPiece S; // the piece moved by one byte
    S.w0 = up ? (A.w0 << 8) | (nb >> 24) : (A.w0 >> 8) | (A.w1 << 24);
    S.w1 = up ? (A.w1 << 8) | (A.w0 >> 24) : (A.w1 >> 8) | (A.w2 << 24);
    S.w2 = up ? (A.w2 << 8) | (A.w1 >> 24) : (A.w2 >> 8) | (A.w3 << 24);
    S.w3 = up ? (A.w3 << 8) | (A.w2 >> 24) : (A.w3 >> 8) | (nb << 24);
    FanoutPiece o;
    o.w0 = red_word(A.w0, S.w0, 16 * q, shift, h, ins);
    o.w1 = red_word(A.w1, S.w1, 16 * q + 4, shift, h, ins);
    o.w2 = red_word(A.w2, S.w2, 16 * q + 8, shift, h, ins);
    o.w3 = red_word(A.w3, S.w3, 16 * q + 12, shift, h, ins);
    o.w0 = q == 0 ? (o.w0 & ~0x00007F00u) | ((pt & 0x7Fu) << 8) : o.w0;
    const bool on = shift != 0;
    o.w0 = on ? o.w0 : A.w0;
    o.w1 = on ? o.w1 : A.w1;
    o.w2 = on ? o.w2 : A.w2;
    o.w3 = on ? o.w3 : A.w3;
    return o;
}

// Byte i of the packet RED left (0 <= i < p.len_out; p.result 1 or 2, else the source's byte).
template <class Rd> SRTP_FANOUT_HD inline int red_byte(Rd rd, int i, const RedPlan &p) {
    if (p.shift == 0) return rd(i);
    const int b = i < p.h ? rd(i) : p.shift > 0 && i == p.h ? p.ins : rd(i - p.shift);
    return i == 1 ? (b & 0x80) | (p.pt & 0x7F) : b;
}

} // namespace srtp
