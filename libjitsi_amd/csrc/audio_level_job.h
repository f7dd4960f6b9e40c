// audio_level_job.h -- what one received entry gets in front of the unprotect
// chain (srtp_transform_device_lvl / _host_lvl): the level of its
// ssrc-audio-level header extension (RFC 6464) and, for a muted source, the
// flag that keeps it from being deciphered.  It is the one engine the
// reference places behind SRTP on the receive side, SsrcTransformEngine
// (MediaStreamImpl.java:1037-1044), restated:
// SsrcTransformEngine.reverseTransform (SsrcTransformEngine.java:226-274) with
// dropMutedAudioSourceInReverseTransform == false, the reference's default
// (:59), over RawPacket.extractSsrcAudioLevel (RawPacket.java:305-318),
// getCsrcAudioLevel (:419-443), findExtension (:331-394),
// getExtensionHeaderLength (:504-524), getExtensionLength (:544-556) and
// getLengthForExtension (:640-648).  Plain functions that the host compiles
// (srtp_audio_level_job, tools/audio_level_check.cpp under AddressSanitizer +
// UBSan) and k_audio_level compiles as they stand: no HIP type and no pointer;
// the packet's bytes come through a byte reader rd(i), byte i of the packet
// (0..255), asked only for 0 <= i < B.  All arithmetic is signed int, and a
// byte is Java's signed byte wherever the reference reads it as one.
//
//   audio_level_wanted(flags, len, cap, ext_id) -> B or 0.  The entry is read
//             only when it is not flagged SKIP, ext_id is in 1..127 (the
//             reference tests `byte ssrcAudioLevelExtID > 0`: a record byte
//             >= 128 is negative as a Java byte, off like 0) and the entry is
//             not isInvalid(): 12 <= len <= cap, neither negative as an int.
//             Then B = len, clamped to 65535 as fanout_clamp does.  Asked
//             before any byte is read: 0 means no byte is.
//   audio_level_find(rd, B, ext_id) -> level: -128 (Byte.MIN_VALUE, "none") or
//             0..127.  (b[0] & 0xC0) >> 6 == 2 (RTPHeader.VERSION), then
//             getExtensionBit, b[0] & 0x10; cc = b[0] & 15;
//               p  = 12 + 4 * cc + 2
//               xl = ((sbyte(b[p]) << 8) | (b[p + 1] & 0xFF)) * 4 -- the first
//                    byte signed, the second not (unlike the abs-send-time
//                    walk); zero or negative: no walk, none
//               getExtensionHeaderLength over b[12 + 4 * cc], b[.. + 1]:
//                    BE DE: the one-byte form; 0x10 and a byte whose signed
//                    >> 4 is 0: the two-byte form; anything else: none
//               o = 12 + 4 * cc + 4; end = o + xl -- the reference does not
//                    bound the walk by the packet's length; while o < end:
//                 one-byte form: type = sbyte(b[o]) >> 4 (-8..7: IDs 8..15
//                    never match), len = (b[o] & 15) + 1, o += 1
//                 two-byte form: type = sbyte(b[o]), len = sbyte(b[o + 1]),
//                    o += 2
//                 the first element whose type equals ext_id ends the walk at
//                    its content, o; otherwise o += len
//               a padding byte is an element of type 0 and len 1: it swallows
//               the byte behind it, as in the reference.  On a match
//               level = 0x7F & b[o]; in the two-byte form a matched element
//               with a negative length byte keeps the default (levelsCount <
//               index).
//             Two places where the reference has no defined answer; here the
//             answer is none, and the packet goes on to SRTP unflagged:
//               * a read at an index >= B.  The reference reads stale bytes of
//                 a larger buffer or throws ArrayIndexOutOfBounds.
//               * a two-byte element that is not the match and has a length
//                 byte >= 0x80.  The reference's offset walks backwards (and
//                 may never end).  With this guard the offset grows by at
//                 least 2 per element, so every walk ends within B / 2 steps.
//   audio_level_flags(caller_flags, level) -> caller_flags | SILENCE when
//             level == 127 (Buffer.FLAG_SILENCE: authenticated, not
//             deciphered, SRTPCryptoContext.java:609), else the caller's
//             flags.  DISCARD and SKIP pass through untouched.
// The rule knows nothing about a transformer's kind: the reference's engine
// has no RTCP transformer, so for SRTCP entries the caller passes ID 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRTP_LEVEL_HD __host__ __device__
#else
#define SRTP_LEVEL_HD
#endif

namespace srtp {

constexpr uint32_t kLvlFlagSkip = 0x80000000u; // SRTP_PKT_FLAG_SKIP (this header stands alone)
constexpr uint32_t kLvlFlagSilence = 0x4u;     // SRTP_PKT_FLAG_SILENCE
constexpr int kLvlMaxRegion = 65535;           // validate_regions: cap <= 65535
constexpr int kLvlHeaderBytes = 12;            // RawPacket.FIXED_HEADER_SIZE
constexpr int kLvlNone = -128;                 // Byte.MIN_VALUE: no level in this packet
constexpr int kLvlMuted = 127;                 // RFC 6464: a muted audio source

SRTP_LEVEL_HD inline int audio_level_sbyte(int b) { return b >= 128 ? b - 256 : b; } // a Java byte

// B, the bytes of the entry the walk may read, or 0: the entry is not read.  ext_id is the record's byte, 0..255.
SRTP_LEVEL_HD inline int audio_level_wanted(uint32_t flags, int len, int cap, int ext_id) {
    if (flags & kLvlFlagSkip) return 0;
    if (ext_id < 1 || ext_id > 127) return 0;
    if (len < 0 || cap < 0) return 0;
    if (len < kLvlHeaderBytes || len > cap) return 0; // RawPacket.isInvalid
    return len > kLvlMaxRegion ? kLvlMaxRegion : len;
}

// The level of the packet's first element of ID ext_id (1..127), or kLvlNone.  B is audio_level_wanted's
// answer, not 0; rd is asked only for 0 <= i < B.
template <class Rd> SRTP_LEVEL_HD inline int audio_level_find(Rd rd, int B, int ext_id) {
    if (B < kLvlHeaderBytes) return kLvlNone;
    const int b0 = rd(0);
    if (((b0 & 0xC0) >> 6) != 2) return kLvlNone; // RTPHeader.VERSION == pkt.getVersion()
    if ((b0 & 0x10) == 0) return kLvlNone;        // getExtensionBit()
    const int x = kLvlHeaderBytes + 4 * (b0 & 15); // behind the CSRCs: "defined by profile"
    if (x + 3 >= B) return kLvlNone;               // the length word lies past the packet
    const int xl = ((audio_level_sbyte(rd(x + 2)) * 256) | rd(x + 3)) * 4; // getExtensionLength()
    if (xl <= 0) return kLvlNone; // 0: nothing there; negative: findExtension's loop never runs
    const int p0 = rd(x), p1 = rd(x + 1);
    int form = 0; // getExtensionHeaderLength()
    if (p0 == 0xBE && p1 == 0xDE)
        form = 1;
    else if (p0 == 0x10 && (audio_level_sbyte(p1) >> 4) == 0)
        form = 2;
    if (form == 0) return kLvlNone;
    int o = x + 4;
    const int end = o + xl; // not bounded by the packet's length, as in the reference
    while (o < end) {
        if (o >= B) return kLvlNone;
        const int e = rd(o);
        int type, len;
        if (form == 1) {
            type = audio_level_sbyte(e) >> 4;
            len = (e & 15) + 1;
            o += 1;
        } else {
            if (o + 1 >= B) return kLvlNone;
            type = audio_level_sbyte(e);
            len = audio_level_sbyte(rd(o + 1));
            o += 2;
        }
        if (type == ext_id) {
            // getLengthForExtension(o) < index 0 only for a two-byte element's negative length byte
            if (len < 0) return kLvlNone;
            if (o >= B) return kLvlNone;
            return 0x7F & rd(o);
        }
        if (len < 0) return kLvlNone; // the reference's offset would walk backwards
        o += len;
    }
    return kLvlNone;
}

SRTP_LEVEL_HD inline uint32_t audio_level_flags(uint32_t caller_flags, int level) {
    return level == kLvlMuted ? caller_flags | kLvlFlagSilence : caller_flags;
}

} // namespace srtp
