// gcm_open_check.cpp -- stand-alone check of the one-pass GCM open's two rules
// (gcm_spec_ok and gcm_fix_action, libjitsi_amd/csrc/gcm_job.h), for a
// sanitizer build (no GPU, no Python).  For every unprotect shape of
// gcm_job_check's sweep -- L in 0..80, the capacities around each trailer
// size, both kinds, the header shapes including negative extension lengths,
// DISCARD, E = 0 / 1 -- it seals a packet with the host aes_gcm into a heap
// buffer of exactly cap bytes, then plays what the kernels do:
//   the open pass   the tag check under the ROC guess g0 and, where
//                   gcm_spec_ok allows, the CTR pass in the same trip, taken
//                   back at once on a mismatch;
//   the walk        every verdict it can give: OK, DROP_REPLAY, DROP_AUTH,
//                   NOT_PROCESSED, ERR_MALFORMED -- on the packet as sealed,
//                   with a flipped tag bit, with a flipped data bit, and
//                   sealed under a ROC other than g0 (which the walk accepts
//                   after its re-check);
//   the fix pass    gcm_fix_action's answer, a CTR pass under the IV of the
//                   speculation and / or one under the walk's.
// and asserts that the buffer ends as the plaintext exactly when the verdict is
// OK and the packet is wanted deciphered, else byte for byte as it came in;
// and that every byte the fix pass reads to rebuild the job and the IV lies
// outside the range the open pass wrote.
//
//   make -C tools gcm_open_check     (built with -fsanitize=address,undefined)
//   tools/gcm_open_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/gcm_job.h"
#include "../libjitsi_amd/csrc/host_crypto.h"

using srtp::GcmJob;

static int failures = 0;
static long cases = 0, played = 0, speculated = 0, restores = 0, lates = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

static uint32_t rk[60];
static int nr;

// the 12 IV bytes: SRTP's carry the ROC, SRTCP's the index (one fixed value here)
static void make_iv(int kind, uint32_t roc, uint8_t iv[12]) {
    for (int i = 0; i < 12; i++) iv[i] = (uint8_t)(0xa0 + i);
    if (kind == 0)
        for (int i = 0; i < 4; i++) iv[6 + i] ^= (uint8_t)(roc >> (24 - 8 * i));
}

// AES-CTR from counter 2 over buf[at, at + n): the decipher pass, and its own inverse
static void ctr_pass(const uint8_t iv[12], uint8_t *buf, int at, int n) {
    for (int b = 0; 16 * b < n; b++) {
        uint8_t ctr[16], ks[16];
        memcpy(ctr, iv, 12);
        const uint32_t c = (uint32_t)b + 2u;
        ctr[12] = (uint8_t)(c >> 24); ctr[13] = (uint8_t)(c >> 16); ctr[14] = (uint8_t)(c >> 8); ctr[15] = (uint8_t)c;
        srtp::aes_encrypt_block_nr(rk, nr, ctr, ks);
        for (int i = 0; i < 16 && 16 * b + i < n; i++) buf[(size_t)(at + 16 * b + i)] ^= ks[i];
    }
}

// a first byte that announces header length h as the sweep's shapes do: plain,
// 2 CSRCs, X with extensions of 0 / 3 words (with and without CSRCs), X with a
// long or a negative extension length, 15 CSRCs and X for the throw mark
static uint32_t byte0_of(int32_t h, int L) {
    if (h == 12) return 0x80u;
    if (h == 20) return 0x82u;
    if (h == 24 || h == 36) return 0x92u;
    if (h == srtp::kGcmHdrThrow) return 0x9Fu;
    (void)L;
    return 0x90u; // 16, 28, L + 4, L + 16, -4, 8, 0
}

enum { kClean = 0, kTagBit = 1, kDataBit = 2, kOtherRoc = 3 };

static void one(int kind, int L, int cap, int32_t h, uint32_t flags, int e) {
    cases++;
    const GcmJob j = srtp::gcm_packet_job(kind, 1, L, cap, h, flags, e);
    const uint32_t b0 = byte0_of(h, L);
    const int spec_ok = srtp::gcm_spec_ok(kind, j, h, b0, e);
    if (j.status != srtp::kGcmNoStatus) {
        CHECK(spec_ok == 0); // the lengths alone settle it: nothing is deciphered, before or after
        return;
    }
    // the rule, restated
    const int fixed = 12 + 4 * (int)(b0 & 15u) + ((b0 & 0x10u) ? 4 : 0);
    CHECK(spec_ok == ((j.decipher && j.data_len > 0 && (kind ? e == 1 : h >= fixed)) ? 1 : 0));
    if (spec_ok) {
        // what the fix pass reads again lies outside the range the open pass wrote
        const int lo = j.data_at, hi = j.data_at + j.data_len;
        auto clear = [&](int a, int b) { return b <= lo || a >= hi; }; // [a, b) against [lo, hi)
        if (kind == 0) {
            CHECK(clear(0, 4));  // V/P/X/CC, M/PT, SEQ
            CHECK(clear(8, 12)); // SSRC
            if (b0 & 0x10u) CHECK(clear(fixed - 4, fixed)); // the extension header
        } else {
            CHECK(clear(4, 8));                       // SSRC
            CHECK(clear(j.word_at, j.word_at + 4));   // the E|index word
        }
        CHECK(clear(j.tag_at, j.tag_at + 16));
    }
    const uint32_t g0 = 7u;
    for (int variant = kClean; variant <= kOtherRoc; variant++) {
        if (variant == kOtherRoc && kind != 0) continue; // SRTCP has no ROC guess
        const uint32_t cw = variant == kOtherRoc ? g0 + 1u : g0; // the ROC the sender used, and the walk finds
        uint8_t iv_g0[12], iv_cw[12];
        make_iv(kind, g0, iv_g0);
        make_iv(kind, cw, iv_cw);
        std::vector<uint8_t> buf((size_t)cap); // heap, exact size: the guard
        for (int i = 0; i < cap; i++) buf[(size_t)i] = (uint8_t)(i * 13 + 5);
        uint8_t word[4] = {(uint8_t)(e ? 0x80 : 0x00), 0, 0, 9};
        if (j.word_at >= 0) memcpy(buf.data() + j.word_at, word, 4);
        const std::vector<uint8_t> plain(buf);
        std::vector<uint8_t> aad(buf.begin(), buf.begin() + j.aad_len);
        if (j.word_aad) aad.insert(aad.end(), word, word + 4);
        uint8_t tag[16];
        CHECK(srtp::aes_gcm(false, rk, nr, iv_cw, aad.data(), aad.size(), buf.data() + j.data_at, (size_t)j.data_len, tag));
        memcpy(buf.data() + j.tag_at, tag, 16);
        if (variant == kTagBit) buf[(size_t)j.tag_at + 5] ^= 4;
        if (variant == kDataBit) {
            if (j.data_len == 0) continue;
            buf[(size_t)(j.data_at + j.data_len / 2)] ^= 0x20;
        }
        const std::vector<uint8_t> came(buf);

        // ---- the open pass, under g0
        std::vector<uint8_t> probe(buf.begin() + j.data_at, buf.begin() + j.data_at + j.data_len);
        const bool tag_ok = srtp::aes_gcm(true, rk, nr, iv_g0, aad.data(), aad.size(), probe.data(), probe.size(),
                                          buf.data() + j.tag_at);
        CHECK(tag_ok == (variant == kClean));
        if (spec_ok) ctr_pass(iv_g0, buf.data(), j.data_at, j.data_len);             // the single trip stores
        if (spec_ok && !tag_ok) ctr_pass(iv_g0, buf.data(), j.data_at, j.data_len);  // ... and is taken back
        const int spec_done = spec_ok && tag_ok;
        if (!spec_done) CHECK(buf == came);
        speculated += spec_done;

        // ---- every verdict of the walk, then the fix pass
        const int verdicts[] = {0, 1, 2, 8, 6};
        for (int st : verdicts) {
            // OK needs a tag the walk can accept: the packet as sealed, under g0 or after the re-check
            if (st == 0 && (variant == kTagBit || variant == kDataBit)) continue;
            played++;
            std::vector<uint8_t> w(buf);
            const int wanted = st == 0 && j.decipher && (kind == 0 || e == 1);
            const int act = srtp::gcm_fix_action(spec_done, st, wanted, kind == 0, g0, cw);
            if (spec_done && wanted) CHECK(act == srtp::kGcmFixNone);
            if (spec_done && !wanted) CHECK(act == srtp::kGcmFixRestore);
            if (!spec_done) CHECK(act == (wanted ? srtp::kGcmFixDecipher : srtp::kGcmFixNone));
            // the fix pass rebuilds the job from the recorded length L and the bytes it re-reads
            const GcmJob f = srtp::gcm_packet_job(kind, 1, L, cap, h, flags, e);
            CHECK(f.data_at == j.data_at && f.data_len == j.data_len);
            if (act & srtp::kGcmFixRestore) { ctr_pass(iv_g0, w.data(), f.data_at, f.data_len); restores++; }
            if (act & srtp::kGcmFixDecipher) { ctr_pass(iv_cw, w.data(), f.data_at, f.data_len); lates++; }
            if (wanted) {
                for (int i = 0; i < cap; i++)
                    CHECK(w[(size_t)i] == (i >= j.data_at && i < j.data_at + j.data_len ? plain[(size_t)i] : came[(size_t)i]));
            } else {
                CHECK(w == came);
            }
        }
        // the case that cannot happen, so that the rule is total: deciphered
        // under g0, accepted under another ROC -- restore, then decipher
        if (variant == kOtherRoc && spec_ok) {
            std::vector<uint8_t> w(came);
            ctr_pass(iv_g0, w.data(), j.data_at, j.data_len);
            const int act = srtp::gcm_fix_action(1, 0, 1, 1, g0, cw);
            CHECK(act == srtp::kGcmFixRestoreDecipher);
            ctr_pass(iv_g0, w.data(), j.data_at, j.data_len);
            ctr_pass(iv_cw, w.data(), j.data_at, j.data_len);
            for (int i = 0; i < cap; i++)
                CHECK(w[(size_t)i] == (i >= j.data_at && i < j.data_at + j.data_len ? plain[(size_t)i] : came[(size_t)i]));
        }
    }
}

int main() {
    uint8_t key[16];
    for (int i = 0; i < 16; i++) key[i] = (uint8_t)(0x51 + 7 * i);
    nr = srtp::aes_expand_le(key, 16, rk);
    for (int L = 0; L <= 80; L++) {
        const int caps[] = {L, L + 15, L + 16, L + 19, L + 20, L + 36};
        const int32_t hs[] = {12, 20, 16, 28, 24, 36, L + 4, L + 16, -4, 8, 0, srtp::kGcmHdrThrow};
        for (int cap : caps)
            for (int kind = 0; kind < 2; kind++)
                for (int32_t h : hs)
                    for (uint32_t fl : {0u, 2u})
                        for (int e = 0; e < 2; e++) one(kind, L, cap, h, fl, e);
    }
    CHECK(speculated > 0 && restores > 0 && lates > 0);
    if (failures) printf("gcm_open_check: %d failures (%ld cases)\n", failures, cases);
    else
        printf("gcm_open_check: ok (%ld cases, %ld verdicts played, %ld speculated, %ld restores, %ld late)\n", cases,
               played, speculated, restores, lates);
    return failures ? 1 : 0;
}
