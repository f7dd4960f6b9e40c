// fec_rx_job.h -- what one record of srtp_fec_recover_device / _host becomes:
// the media packet that one ulpfec packet (RFC 5109, one level, short or long
// mask) and up to 64 candidate entries of the same tables give back, or the
// reason why none is made.  Plain functions that the host compiles
// (srtp_fec_recover_job, the host route's checks, tools/fec_recover_check.cpp
// under AddressSanitizer + UBSan) and k_fec_recover compiles as they stand: no
// HIP type and no pointer.  The FEC packet's header comes through a byte reader
// rd(i), byte i of the packet, asked only for 0 <= i < len; the packets' bodies
// come in as aligned little-endian words that the caller loaded; which piece
// and which word to load is said here, and every byte at or past an entry's len
// is masked off before it is used, so a caller may load whatever lies between
// len and len rounded up to 16 and nothing past that.  All arithmetic is signed
// int, uint32 or (the mask) uint64.
//
// The reference, restated: FECReceiver.Reconstructor (transform/fec/
// FECReceiver.java), setFecPacket (:472-520) and recover (:527-596), over
// RawPacket.getHeaderLength (red_header_length, red_job.h).
//   setFecPacket  idx = getHeaderLength() = hl; maskLen = (b[hl] & 0x40) == 0 ?
//             2 : 6; base = u16 at hl + 2; the mask's bytes are b[hl + 12 ..];
//             bit j of byte i (1 << (7 - j)) stands for the key base + 8 i + j,
//             an int that is NOT reduced mod 2^16: mediaPackets.get() of a key
//             above 65535 finds nothing, and the packet counts as missing.  So
//             a complete group that crosses the wrap with one key past 65535
//             "recovers" a duplicate of a packet that was received, and with
//             two or more such keys waits for ever.  Kept.  A key that is found
//             joins neededPackets; numMissing counts the others, sequenceNumber
//             is the last of them.  (The loop leaves at numMissing > 1; nothing
//             reads what it leaves unfinished.)
//   the verdict   numMissing == 0: the FEC packet is of no further use
//             (kFecRxComplete); > 1: kFecRxWait; == 1: recover().
//   recover   lengthRecovery = (u16 at hl + 8 ^ XOR of (len - 12) over the
//             needed packets) & 0xFFFF; the new packet has lengthRecovery + 12
//             bytes; bytes 0..7 = FEC bytes hl .. hl + 7 ^ the needed packets'
//             bytes 0..7; byte 0 = (b & 0x3F) | 0x80; protectionLength = u16 at
//             hl + 10; protectionLength < lengthRecovery: "Recovered only a
//             partial RTP packet", null (kFecRxPartial); bytes 12 .. = FEC
//             bytes hl + 14 .. (hl + 18 .. with the long mask), each needed
//             packet's bytes i in [12, min(lengthRecovery + 12, len)) XORed in;
//             setSSRC: bytes 8..11; setSequenceNumber: bytes 2..3 = key &
//             0xFFFF.
//   mediaPackets  a TreeMap by sequence number: of candidates with equal keys
//             the one latest in the list stands (put replaces).
//
// Defined deviations (the reference reads the stale bytes of a larger buffer or
// throws): the record is kFecRxRefused when a read of the FEC packet would fall
// at or past its len -- the extension length (red_header_length's oob), hl < 0,
// hl + 14 > len, hl + 18 > len with the long mask -- and, for a recovery, when
// payload start + lengthRecovery > len.  The order is the reference's: partial
// is asked before the payload is copied.
//
//   fecrx_record_ok   the record's own fields: count <= 64 (MEDIA_BUF_SIZE),
//             first + count <= n_cand.
//   fecrx_index_ok, fecrx_entry_ok   an entry, the FEC packet or a candidate,
//             counts iff its index lies in [0, n), its status is OK and 12 <=
//             len <= cap <= 65535.  Asked in this order: the index before
//             anything of the entry is read, status and lengths before its
//             first byte.  A candidate that fails is absent (a packet that
//             failed authentication was not received), which is no refusal; the
//             FEC entry that fails refuses the record.
//   fecrx_head    the FEC header's scalars, or refused.
//   fecrx_bit     the mask bit a candidate's key stands for, or -1.
//   fecrx_take    the needed set, walked from the last candidate to the first:
//             a key that is covered already drops the earlier candidate.
//   fecrx_plan    the code, the key and the lengths.
//
// Geometry.  Regions start 16-byte aligned.  Media contributions are aligned:
// output byte d takes member byte d, so piece q of the packet needs of each
// needed member its piece q (piece 0, masked to nothing, where 16 q >= len).
// The FEC packet's contribution is shifted: output byte d >= 12 is FEC byte d +
// hl + 2 (+ 6 with the long mask); hl is a multiple of 4, so the shift is 2 mod
// 4: piece q needs the five consecutive aligned words from FEC byte 16 q + hl
// (+ 4) on, funnelled down by two bytes (fecrx_fec_word, fecrx_piece); a word
// that does not start below len is named word 0 and masked.  Output bytes 0..7
// are FEC bytes hl .. hl + 7, unshifted (FecRxHead.h0, h1), and bytes 8..11 the
// record's SSRC: piece 0 replaces its words 0..2.  Every load is an aligned
// 16-byte piece or an aligned 4-byte word that starts below the entry's len,
// hence below len rounded up to 16, which its region owns.  Stores stay below
// fecrx_store_bytes = min(len_out, out_cap) rounded up to 16, and only where
// that fits out_cap rounded up to 16.  (Nothing of fec_job.h is used here: a
// second device-side caller of its helpers changes how the compiler inlines
// them into k_fanout_fec, and with that the code of a kernel this header has
// no business with.)
#pragma once
#include "red_job.h"

namespace srtp {

constexpr int kFecRxOff = 0, kFecRxRecovered = 1, kFecRxComplete = 2, kFecRxWait = 3, kFecRxPartial = 4,
              kFecRxRefused = -1;  // SRTP_FECRX_*
constexpr int kFecRxMaxCandidates = 64; // FECReceiver.MEDIA_BUF_SIZE
constexpr int kFecRxStatusOk = 0, kFecRxStatusInvalid = 7, kFecRxStatusSkipped = 9; // SRTP_STATUS_*

SRTP_FANOUT_HD inline bool fecrx_record_ok(uint32_t first, uint32_t count, uint32_t n_cand) {
    return count <= (uint32_t)kFecRxMaxCandidates && first <= n_cand && count <= n_cand - first;
}
SRTP_FANOUT_HD inline bool fecrx_index_ok(int i, int n) { return i >= 0 && i < n; }
SRTP_FANOUT_HD inline bool fecrx_entry_ok(int status, int len, int cap) {
    return status == kFecRxStatusOk && len >= kFanHeaderBytes && cap >= 0 && cap <= kFanMaxRegion && len <= cap;
}
// w0: the entry's bytes 0..3, little-endian -> its sequence number
SRTP_FANOUT_HD inline int fecrx_key(uint32_t w0) { return (int)((((w0 >> 16) & 0xFFu) << 8) | (w0 >> 24)); }

struct FecRxHead {
    int code;      // 0, or kFecRxRefused
    int hl;        // getHeaderLength(): a multiple of 4, 0 <= hl <= len - 14
    int lm;        // 0, or 4 with the long mask
    int nbits;     // 16 or 48
    int base;      // SN base
    uint64_t mask; // bit k: the key base + k is protected
    int len_rec;   // the length recovery field
    int plen;      // the protection length
    uint32_t h0, h1; // FEC bytes hl .. hl + 7 as two words
};

template <class Rd> SRTP_FANOUT_HD inline uint32_t fecrx_word(Rd rd, int i) {
    return (uint32_t)rd(i) | ((uint32_t)rd(i + 1) << 8) | ((uint32_t)rd(i + 2) << 16) | ((uint32_t)rd(i + 3) << 24);
}

// len: the FEC entry's, fecrx_entry_ok passed (12 <= len <= 65535).
template <class Rd> SRTP_FANOUT_HD inline FecRxHead fecrx_head(Rd rd, int len) {
    FecRxHead h;
    h.code = kFecRxRefused;
    h.hl = 0; h.lm = 0; h.nbits = 0; h.base = 0; h.mask = 0ull; h.len_rec = 0; h.plen = 0; h.h0 = 0u; h.h1 = 0u;
    bool oob;
    const int hl = red_header_length(rd, len, oob);
    if (oob || hl < 0 || hl + 14 > len) return h;
    const int b = rd(hl);
    const bool lng = (b & 0x40) != 0;
    if (lng && hl + 18 > len) return h;
    h.hl = hl;
    h.lm = lng ? 4 : 0;
    h.nbits = lng ? 48 : 16;
    h.base = (rd(hl + 2) << 8) | rd(hl + 3);
    h.len_rec = (rd(hl + 8) << 8) | rd(hl + 9);
    h.plen = (rd(hl + 10) << 8) | rd(hl + 11);
    uint64_t m = 0ull;
    for (int i = 0; i < (lng ? 6 : 2); i++) {
        const int mb = rd(hl + 12 + i);
        for (int j = 0; j < 8; j++)
            if (mb & (1 << (7 - j))) m |= 1ull << (8 * i + j);
    }
    h.mask = m;
    h.h0 = fecrx_word(rd, hl);
    h.h1 = fecrx_word(rd, hl + 4);
    h.code = 0;
    return h;
}

// The mask bit that a present candidate's key stands for, or -1: mediaPackets.get(base + k) finds it.
SRTP_FANOUT_HD inline int fecrx_bit(int key, const FecRxHead &h) {
    const int d = key - h.base;
    return d >= 0 && d < h.nbits && ((h.mask >> d) & 1ull) ? d : -1;
}
// Candidates are asked from the last of the list to the first: true where this one's packet is the map's.
SRTP_FANOUT_HD inline bool fecrx_take(uint64_t &covered, int d) {
    if (d < 0 || ((covered >> d) & 1ull)) return false;
    covered |= 1ull << d;
    return true;
}

struct FecRxPlan {
    int code;    // kFecRxRecovered, Complete, Wait, Partial or Refused
    int key;     // the missing key (base + k, up to 65535 + 47) where numMissing == 1
    int lr;      // lengthRecovery
    int len_out; // lengthRecovery + 12 where recovered, else 0
};

SRTP_FANOUT_HD inline int fecrx_popcount(uint64_t v) {
    int c = 0;
    for (; v; v &= v - 1ull) c++;
    return c;
}
// len_xor: the XOR of len - 12 over the needed packets; fec_len: the FEC entry's len.
SRTP_FANOUT_HD inline FecRxPlan fecrx_plan(const FecRxHead &h, uint64_t covered, int len_xor, int fec_len) {
    FecRxPlan p;
    p.key = 0; p.lr = 0; p.len_out = 0;
    const uint64_t missing = h.mask & ~covered;
    const int nm = fecrx_popcount(missing);
    p.code = nm == 0 ? kFecRxComplete : kFecRxWait;
    if (nm != 1) return p;
    int k = 0;
    while (!((missing >> k) & 1ull)) k++;
    p.key = h.base + k;
    p.lr = (h.len_rec ^ len_xor) & 0xFFFF;
    p.code = kFecRxPartial;
    if (h.plen < p.lr) return p;
    p.code = kFecRxRefused;
    if (h.hl + 14 + h.lm + p.lr > fec_len) return p;
    p.code = kFecRxRecovered;
    p.len_out = p.lr + kFanHeaderBytes;
    return p;
}
// out_status of a record: OK, DROP_INVALID (longer than its region) or SKIPPED (nothing recovered)
SRTP_FANOUT_HD inline int fecrx_status(const FecRxPlan &p, int out_cap) {
    if (p.code != kFecRxRecovered) return kFecRxStatusSkipped;
    return out_cap >= 0 && p.len_out <= fanout_clamp(out_cap) ? kFecRxStatusOk : kFecRxStatusInvalid;
}

// The bytes of a word at byte `at` of an entry that lie below its len.
SRTP_FANOUT_HD inline uint32_t fecrx_mask(int at, int len) {
    const int r = len - at;
    return r <= 0 ? 0u : r >= 4 ? 0xFFFFFFFFu : (1u << (8 * r)) - 1u;
}
// Which aligned piece of a needed member feeds output piece q (len >= 12, or 0: nothing).
SRTP_FANOUT_HD inline int fecrx_src_piece(int q, int len) { return 16 * q < len ? q : 0; }
// The FEC byte at which word i (0..4) of output piece q's window starts, and the word to load for it.
SRTP_FANOUT_HD inline int fecrx_fec_at(int q, int i, const FecRxHead &h) { return 16 * q + 4 * i + h.hl + h.lm; }
SRTP_FANOUT_HD inline int fecrx_fec_word(int q, int i, const FecRxHead &h, int fec_len) {
    const int at = fecrx_fec_at(q, i, h);
    return at < fec_len ? at / 4 : 0;
}

SRTP_FANOUT_HD inline uint32_t fecrx_be16(uint32_t v) { return ((v >> 8) & 0xFFu) | ((v & 0xFFu) << 8); }
// two bytes down: the upper half of lo under the lower half of hi
SRTP_FANOUT_HD inline uint32_t fecrx_funnel(uint32_t lo, uint32_t hi) { return (lo >> 16) | (hi << 16); }
// How many bytes of the packet are stored: below min(len_out, cap) rounded up to 16, which a region owns.
SRTP_FANOUT_HD inline int fecrx_store_bytes(int len_out, int out_cap) {
    if (len_out < 0 || out_cap < 0) return 0;
    const int oc = fanout_clamp(out_cap);
    const int c = len_out < oc ? len_out : oc;
    const int store = (c + 15) & ~15;
    return store <= ((oc + 15) & ~15) ? store : 0;
}

struct FecRxWindow {
    uint32_t w0, w1, w2, w3; // the needed members' piece q, masked, XORed
};
// P: the member's piece fecrx_src_piece(q, len).  len 0: nothing.
SRTP_FANOUT_HD inline void fecrx_accumulate(FecRxWindow &a, const FanoutPiece &P, int q, int len) {
    const int at = 16 * q;
    a.w0 ^= P.w0 & fecrx_mask(at, len);
    a.w1 ^= P.w1 & fecrx_mask(at + 4, len);
    a.w2 ^= P.w2 & fecrx_mask(at + 8, len);
    a.w3 ^= P.w3 & fecrx_mask(at + 12, len);
}

// Piece q of the recovered packet.  F0..F4: the FEC words fecrx_fec_word(q, 0..4) as loaded.
SRTP_FANOUT_HD inline FanoutPiece fecrx_piece(const FecRxWindow &a, uint32_t F0, uint32_t F1, uint32_t F2, uint32_t F3,
                                              uint32_t F4, int q, const FecRxHead &h, const FecRxPlan &p, int fec_len,
                                              uint32_t ssrc) {
    F0 &= fecrx_mask(fecrx_fec_at(q, 0, h), fec_len);
    F1 &= fecrx_mask(fecrx_fec_at(q, 1, h), fec_len);
    F2 &= fecrx_mask(fecrx_fec_at(q, 2, h), fec_len);
    F3 &= fecrx_mask(fecrx_fec_at(q, 3, h), fec_len);
    F4 &= fecrx_mask(fecrx_fec_at(q, 4, h), fec_len);
    FanoutPiece o;
    o.w0 = fecrx_funnel(F0, F1) ^ a.w0;
    o.w1 = fecrx_funnel(F1, F2) ^ a.w1;
    o.w2 = fecrx_funnel(F2, F3) ^ a.w2;
    o.w3 = fecrx_funnel(F3, F4) ^ a.w3;
    if (q == 0) { // the header: FEC bytes hl .. hl + 7 unshifted, version 2, the key and the SSRC
        const uint32_t x0 = h.h0 ^ a.w0;
        o.w0 = (x0 & 0x0000FF3Fu) | 0x80u | (fecrx_be16((uint32_t)p.key & 0xFFFFu) << 16);
        o.w1 = h.h1 ^ a.w1;
        o.w2 = fanout_be32(ssrc);
    }
    return o;
}

} // namespace srtp
