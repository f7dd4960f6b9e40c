// gcm_job.h -- the stateless geometry of one packet under the RFC 7714 AES-GCM
// profiles: which status a packet gets from its lengths alone, and otherwise
// where its AAD, data, tag and E|index word lie.  One plain function that the
// host compiles (srtp_gcm_packet_job, tools/gcm_job_check.cpp under
// AddressSanitizer + UBSan) and a gfx950 kernel can compile as it stands
// (SRTP_GCM_HD; no HIP type, no pointer): every offset a GCM pass forms comes
// from here, and a range is handed out only after it is shown to lie inside
// [0, cap).  All arithmetic is signed int on values already bounded by cap.
//
// The rules are tests/gcm_ref.py process_one's (T = 16):
//   SRTP protect:    L + 16 > cap -> ERR_CAPACITY; h thrown, negative or > L
//                    -> ERR_MALFORMED; AAD [0, h), data [h, L), tag at L.
//   SRTP unprotect:  h thrown or negative -> ERR_MALFORMED; L - 16 < h ->
//                    DROP_AUTH with length max(0, L - 16); AAD [0, h), data
//                    [h, L - 16), tag at L - 16.
//   SRTCP protect:   L + 20 > cap -> ERR_CAPACITY; AAD [0, 8) || the E|index
//                    word, written at L + 16; data [8, L); tag at L.
//   SRTCP unprotect: L < 20 -> ERR_MALFORMED; L < 28 -> DROP_AUTH with length
//                    L - 20; the word is read at L - 4; E = 1: AAD [0, 8) ||
//                    word, data [8, L - 20); E = 0 (RFC 7714 9.3): AAD
//                    [0, L - 20) || word, no data; tag at L - 20.
// Where the stateful checks sit between these is the walk's business:
// ERR_CAPACITY precedes every state change; SRTP's replay check precedes its
// ERR_MALFORMED / DROP_AUTH; SRTCP's follows them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRTP_GCM_HD __host__ __device__
#else
#define SRTP_GCM_HD
#endif

namespace srtp {

constexpr int kGcmTag = 16;
constexpr int32_t kGcmHdrThrow = (int32_t)0x80000000; // the header length could not be read (kHdrThrow)
constexpr int kGcmNoStatus = -1;

// statuses and flags as include/srtp_mi355x.h names them (this header stands alone)
constexpr int kGcmStDropAuth = 2, kGcmStCapacity = 5, kGcmStMalformed = 6, kGcmStInvalid = 7,
              kGcmStInternal = 10;
constexpr uint32_t kGcmFlagNoDecipher = 0x2u | 0x4u; // SRTP_PKT_FLAG_DISCARD | _SILENCE

// The room behind a packet that protect may need on the per-packet paths
// (aggregator, queue, RawPacket batch): SRTCP's E|index word and a 12-byte
// tag, or, on an engine whose AES-GCM switch is on, GCM SRTCP's 16-byte tag
// and the word (the SRTCP protect rule below).
SRTP_GCM_HD inline uint32_t trailer_room(int aead) { return aead ? (uint32_t)kGcmTag + 4u : 16u; }

struct GcmJob {
    int32_t status;   // kGcmNoStatus, or the status the lengths alone decide (then no range is valid)
    int32_t new_len;  // the length the packet leaves with (under `status`, or when accepted)
    int32_t aad_len;  // head AAD: [0, aad_len)
    int32_t word_at;  // the E|index word: -1 none; unprotect: read here; protect: written here
    int32_t word_aad; // 1: the word is AAD too, behind the head AAD
    int32_t data_at;  // data: [data_at, data_at + data_len), seal / decipher in place
    int32_t data_len;
    int32_t tag_at;   // the 16-byte tag: [tag_at, tag_at + 16)
    int32_t decipher; // unprotect: 0 = verify only (DISCARD / SILENCE); else 1
};

SRTP_GCM_HD inline GcmJob gcm_job_early(int status, int new_len) {
    GcmJob j;
    j.status = status;
    j.new_len = new_len;
    j.aad_len = 0;
    j.word_at = -1;
    j.word_aad = 0;
    j.data_at = 0;
    j.data_len = 0;
    j.tag_at = -1;
    j.decipher = 0;
    return j;
}

// kind: 0 SRTP, 1 SRTCP.  reverse: 0 protect, 1 unprotect.  h: the RTP header
// length (RawPacket.getHeaderLength) or kGcmHdrThrow; ignored for SRTCP.
// e_bit: SRTCP unprotect only, the word's E bit (the word's place does not
// depend on it: ask with any value, read the word, ask again).
SRTP_GCM_HD inline GcmJob gcm_packet_job(int kind, int reverse, int L, int cap, int32_t h, uint32_t flags,
                                         int e_bit) {
    if (L < 12 || L > cap) return gcm_job_early(kGcmStInvalid, L); // RawPacket.isInvalid
    // from here 12 <= L <= cap: cap - L cannot overflow, nor any sum below
    GcmJob j = gcm_job_early(kGcmNoStatus, L);
    j.decipher = 1;
    const bool h_bad = h == kGcmHdrThrow || h < 0;
    if (kind == 0) {
        if (!reverse) {
            if (cap - L < kGcmTag) return gcm_job_early(kGcmStCapacity, L);
            if (h_bad || h > L) return gcm_job_early(kGcmStMalformed, L);
            j.aad_len = h;
            j.data_at = h;
            j.data_len = L - h;
            j.tag_at = L;
            j.new_len = L + kGcmTag;
        } else {
            if (h_bad) return gcm_job_early(kGcmStMalformed, L);
            if (L - kGcmTag < h) return gcm_job_early(kGcmStDropAuth, L - kGcmTag > 0 ? L - kGcmTag : 0);
            j.aad_len = h;
            j.data_at = h;
            j.data_len = L - kGcmTag - h;
            j.tag_at = L - kGcmTag;
            j.new_len = L - kGcmTag;
            j.decipher = (flags & kGcmFlagNoDecipher) ? 0 : 1;
        }
    } else {
        if (!reverse) {
            if (cap - L < kGcmTag + 4) return gcm_job_early(kGcmStCapacity, L);
            j.aad_len = 8;
            j.data_at = 8;
            j.data_len = L - 8;
            j.tag_at = L;
            j.word_at = L + kGcmTag;
            j.word_aad = 1;
            j.new_len = L + kGcmTag + 4;
        } else {
            if (L < kGcmTag + 4) return gcm_job_early(kGcmStMalformed, L);
            if (L < 8 + kGcmTag + 4) return gcm_job_early(kGcmStDropAuth, L - kGcmTag - 4);
            const int end = L - kGcmTag - 4;
            j.aad_len = e_bit ? 8 : end;
            j.data_at = e_bit ? 8 : end;
            j.data_len = e_bit ? end - 8 : 0;
            j.tag_at = end;
            j.word_at = L - 4;
            j.word_aad = 1;
            j.new_len = end;
        }
    }
    // The proof, once more, on what is about to be handed out: ordered ranges
    // AAD | data | tag (| word), all inside [0, cap).  It cannot fail by the
    // branches above; should an edit break one, the packet is refused here
    // and no offset leaves.
    const bool ok = j.aad_len >= 0 && j.data_at == j.aad_len && j.data_len >= 0 &&
                    j.data_at + j.data_len == j.tag_at && j.tag_at + kGcmTag <= cap &&
                    (j.word_at < 0 || (j.word_at == j.tag_at + kGcmTag && j.word_at + 4 <= cap)) &&
                    j.new_len >= 0 && j.new_len <= cap;
    if (!ok) return gcm_job_early(kGcmStInternal, L);
    return j;
}

// ---- the one-pass open (k_gcm<kGcmOpen> / <kGcmFix>, the wave kernels' twins)
// The pass before the walk checks a packet's tag under the ROC guess g0 (SRTCP:
// under its index word) and, where gcm_spec_ok allows, deciphers it in the same
// trip; the pass after the walk compares that with the walk's verdict and
// repairs the misses (gcm_fix_action).  Both rules in one place, for the
// kernels and for tools/gcm_open_check.cpp.

// May the open pass decipher this unprotect packet before the walk?  j: its
// job (gcm_packet_job with reverse = 1 and, for SRTCP, the word's E bit); h: the
// RTP header length the job was asked with; b0: the packet's first byte (CC in
// bits 0-3, X in bit 4); e_bit: SRTCP's E bit.  The SRTP rule is k_unprotect's:
// a negative extension length can give a header length below the fixed header
// 12 + 4 CC (+ 4 with X), which puts bytes the fix pass re-reads (byte 0, the
// extension length, the SSRC) inside the deciphered range -- such a packet is
// only verified, and deciphered after the walk.
SRTP_GCM_HD inline int gcm_spec_ok(int kind, const GcmJob &j, int32_t h, uint32_t b0, int e_bit) {
    if (j.status != kGcmNoStatus || !j.decipher || j.data_len <= 0) return 0;
    if (kind != 0) return e_bit ? 1 : 0;
    const int fixed = 12 + 4 * (int)(b0 & 0x0fu) + ((b0 & 0x10u) ? 4 : 0);
    return h != kGcmHdrThrow && h >= fixed ? 1 : 0;
}

// What the fix pass owes a packet: bit 0 (kGcmFixRestore) the CTR pass again
// under the IV of the speculation (g0 / the index word) over the length the
// packet came with, which puts the ciphertext back; bit 1 (kGcmFixDecipher)
// the decipher under the walk's ROC w_cw, today's k_gcm<kGcmDecipher> step.
constexpr int kGcmFixNone = 0, kGcmFixRestore = 1, kGcmFixDecipher = 2, kGcmFixRestoreDecipher = 3;

// spec_done: the open pass deciphered the packet (its tag matched under g0).
// wanted: final status OK, the job's `decipher` set and, for SRTCP, E = 1.
// rtp: SRTP (g0 and cw are ROCs; for SRTCP they play no part).  A speculation
// that the walk confirms under another ROC cannot happen -- a tag that matches
// under g0 proves g0 -- and still gets restore, then decipher.
SRTP_GCM_HD inline int gcm_fix_action(int spec_done, int final_status, int wanted, int rtp, uint32_t g0,
                                      uint32_t cw) {
    const bool want = wanted && final_status == 0;
    if (spec_done) {
        if (!want) return kGcmFixRestore;
        return rtp && g0 != cw ? kGcmFixRestoreDecipher : kGcmFixNone;
    }
    return want ? kGcmFixDecipher : kGcmFixNone;
}

} // namespace srtp
