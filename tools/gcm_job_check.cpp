// gcm_job_check.cpp -- stand-alone check of gcm_packet_job (libjitsi_amd/csrc/
// gcm_job.h), the one function every GCM pass of the engine takes its packet
// offsets from, for a sanitizer build (no GPU, no Python): sweeps it over
// every length 0..80, the capacities around each trailer size, both kinds and
// directions, the header shapes that matter (plain, CSRCs, extensions of 0 and
// 3 words, extensions past the packet, a negative one, the throw mark), the
// DISCARD flag and E = 0 / 1; asserts that every range handed out is ordered,
// inside [0, cap) and clear of the tag; then replays the case with the host
// aes_gcm on a heap buffer of exactly cap bytes, so that AddressSanitizer sees
// any byte outside it.
//
//   make -C tools gcm_job_check      (built with -fsanitize=address,undefined)
//   tools/gcm_job_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/gcm_job.h"
#include "../libjitsi_amd/csrc/host_crypto.h"

using srtp::GcmJob;

static int failures = 0;
static long cases = 0, replayed = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

// the statuses tests/gcm_ref.py process_one gives from the lengths alone
static int expect_status(int kind, int rev, int L, int cap, int32_t h, int *len) {
    *len = L;
    if (L < 12 || L > cap) return 7;
    const bool bad = h == srtp::kGcmHdrThrow || h < 0;
    if (kind == 0) {
        if (!rev) return L + 16 > cap ? 5 : (bad || h > L) ? 6 : -1;
        if (bad) return 6;
        if (L - 16 < h) { *len = L - 16 > 0 ? L - 16 : 0; return 2; }
        return -1;
    }
    if (!rev) return L + 20 > cap ? 5 : -1;
    if (L < 20) return 6;
    if (L < 28) { *len = L - 20; return 2; }
    return -1;
}

static void one(int kind, int rev, int L, int cap, int32_t h, uint32_t flags, int e) {
    cases++;
    const GcmJob j = srtp::gcm_packet_job(kind, rev, L, cap, h, flags, e);
    int want_len;
    const int want = expect_status(kind, rev, L, cap, h, &want_len);
    CHECK(j.status == want);
    if (j.status != srtp::kGcmNoStatus) {
        CHECK(j.new_len == want_len);
        CHECK(j.tag_at == -1 && j.word_at == -1 && j.aad_len == 0 && j.data_len == 0); // no range leaves
        return;
    }
    // ordered, inside [0, cap), clear of the tag
    CHECK(j.aad_len >= 0 && j.aad_len <= cap);
    CHECK(j.data_at >= j.aad_len && j.data_len >= 0 && j.data_at + j.data_len <= cap);
    CHECK(j.tag_at >= j.data_at + j.data_len && j.tag_at >= j.aad_len && j.tag_at + 16 <= cap);
    if (j.word_at >= 0) CHECK(j.word_at >= j.tag_at + 16 && j.word_at + 4 <= cap && j.word_aad == 1);
    else CHECK(kind == 0 && j.word_aad == 0);
    CHECK(j.new_len >= 0 && j.new_len <= cap);
    CHECK(j.new_len == (rev ? L - (kind ? 20 : 16) : L + (kind ? 20 : 16)));
    if (kind == 0) CHECK(j.aad_len == h && j.data_at == h);
    else CHECK(j.aad_len == ((rev && !e) ? L - 20 : 8) && (rev ? j.word_at == L - 4 : j.word_at == L + 16));
    CHECK(j.decipher == ((kind == 0 && rev && (flags & 6u)) ? 0 : 1));
    if (failures) return;

    // replay on a buffer of exactly cap bytes: protect seals through the job's
    // ranges; unprotect first builds the sealed packet the same way
    replayed++;
    uint8_t key[16], iv[12];
    for (int i = 0; i < 16; i++) key[i] = (uint8_t)(0x51 + 7 * i);
    for (int i = 0; i < 12; i++) iv[i] = (uint8_t)(0xa0 + i);
    uint32_t rk[60];
    const int nr = srtp::aes_expand_le(key, 16, rk);
    std::vector<uint8_t> buf((size_t)cap); // heap, exact size: the guard
    for (int i = 0; i < cap; i++) buf[(size_t)i] = (uint8_t)(i * 13 + 5);
    const std::vector<uint8_t> before(buf);
    uint8_t word[4] = {(uint8_t)(e ? 0x80 : 0x00), 0, 0, 9};
    if (j.word_at >= 0 && rev) memcpy(buf.data() + j.word_at, word, 4);
    // the AAD: head || word (the kernels splice the word in without a copy; a
    // copy of the AAD alone serves here)
    std::vector<uint8_t> aad(buf.begin(), buf.begin() + j.aad_len);
    if (j.word_aad) aad.insert(aad.end(), word, word + 4);
    uint8_t tag[16];
    if (!rev) {
        CHECK(srtp::aes_gcm(false, rk, nr, iv, aad.data(), aad.size(), buf.data() + j.data_at, (size_t)j.data_len, tag));
        memcpy(buf.data() + j.tag_at, tag, 16);
        if (j.word_at >= 0) memcpy(buf.data() + j.word_at, word, 4);
        // only [data, new_len) changed
        for (int i = 0; i < cap; i++)
            if (i < j.data_at || i >= j.new_len) CHECK(buf[(size_t)i] == before[(size_t)i]);
        // ... and it opens again through the unprotect job of the new length
        const GcmJob u = srtp::gcm_packet_job(kind, 1, j.new_len, cap, h, 0u, 1);
        CHECK(u.status == srtp::kGcmNoStatus && u.tag_at == j.tag_at && u.data_at == j.data_at &&
              u.data_len == j.data_len && u.word_at == j.word_at && u.new_len == L);
        CHECK(srtp::aes_gcm(true, rk, nr, iv, aad.data(), aad.size(), buf.data() + u.data_at, (size_t)u.data_len,
                            buf.data() + u.tag_at));
        for (int i = 0; i < L; i++) CHECK(buf[(size_t)i] == before[(size_t)i]);
    } else {
        // seal what the job calls data, put the tag where it says, then open
        CHECK(srtp::aes_gcm(false, rk, nr, iv, aad.data(), aad.size(), buf.data() + j.data_at, (size_t)j.data_len, tag));
        memcpy(buf.data() + j.tag_at, tag, 16);
        const std::vector<uint8_t> sealed(buf);
        if (j.decipher) {
            CHECK(srtp::aes_gcm(true, rk, nr, iv, aad.data(), aad.size(), buf.data() + j.data_at, (size_t)j.data_len,
                                buf.data() + j.tag_at));
            for (int i = 0; i < j.new_len; i++) CHECK(buf[(size_t)i] == before[(size_t)i]);
        }
        buf = sealed;
        buf[(size_t)j.tag_at + 5] ^= 4; // a forged tag: refused, nothing written
        CHECK(!srtp::aes_gcm(true, rk, nr, iv, aad.data(), aad.size(), buf.data() + j.data_at, (size_t)j.data_len,
                             buf.data() + j.tag_at));
        buf[(size_t)j.tag_at + 5] ^= 4;
        CHECK(buf == sealed);
    }
}

int main() {
    for (int L = 0; L <= 80; L++) {
        const int caps[] = {L, L + 15, L + 16, L + 19, L + 20, L + 36};
        // header lengths: 12 plain; 12 + 2 CSRCs; extensions of 0 and 3 words
        // (with and without CSRCs); an extension longer than the packet by 4
        // and by 16; a negative extension (a negative and a small positive
        // header length); the throw mark
        const int32_t hs[] = {12, 20, 16, 28, 24, 36, L + 4, L + 16, -4, 8, 0, srtp::kGcmHdrThrow};
        for (int cap : caps)
            for (int kind = 0; kind < 2; kind++)
                for (int rev = 0; rev < 2; rev++)
                    for (int32_t h : hs)
                        for (uint32_t fl : {0u, 2u})
                            for (int e = 0; e < 2; e++) one(kind, rev, L, cap, h, fl, e);
    }
    // lengths and capacities at the ends of the int range
    for (int L : {-1, -2147483647 - 1, 2147483647})
        for (int cap : {0, 65535, 2147483647, -1})
            for (int kind = 0; kind < 2; kind++)
                for (int rev = 0; rev < 2; rev++) {
                    const GcmJob j = srtp::gcm_packet_job(kind, rev, L, cap, 12, 0u, 1);
                    CHECK(j.status != srtp::kGcmNoStatus || (L >= 12 && L <= cap));
                }
    {
        const GcmJob j = srtp::gcm_packet_job(1, 0, 2147483647, 2147483647, 12, 0u, 1);
        CHECK(j.status == 5);
        const GcmJob k = srtp::gcm_packet_job(0, 1, 2147483647, 2147483647, 2147483647, 0u, 1);
        CHECK(k.status == 2 && k.new_len == 2147483647 - 16);
    }
    if (failures) printf("gcm_job_check: %d failures (%ld cases)\n", failures, cases);
    else printf("gcm_job_check: ok (%ld cases, %ld replayed)\n", cases, replayed);
    return failures ? 1 : 0;
}
