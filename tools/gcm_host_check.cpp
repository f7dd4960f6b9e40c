// gcm_host_check.cpp -- stand-alone check of the host AES-GCM code for a
// sanitizer build (no GPU, no Python): links host_crypto.cpp and runs the
// NIST known answers, seal / open round trips over the odd AAD and data
// lengths the tests use, and the RFC 7714 key derivation.
//
//   make -C tools gcm_host_check      (built with -fsanitize=address,undefined)
//   tools/gcm_host_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/host_crypto.h"

static int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);      \
            failures++;                                              \
        }                                                            \
    } while (0)

static std::vector<uint8_t> hex(const char *s) {
    std::vector<uint8_t> v;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        unsigned b = 0;
        sscanf(s + i, "%2x", &b);
        v.push_back((uint8_t)b);
    }
    return v;
}

static bool gcm(bool open, const uint8_t *key, int klen, const uint8_t iv[12], const uint8_t *aad, size_t alen,
                uint8_t *data, size_t len, uint8_t tag[16]) {
    uint32_t rk[60];
    const int nr = srtp::aes_expand_le(key, klen, rk);
    return srtp::aes_gcm(open, rk, nr, iv, aad, alen, data, len, tag);
}

int main() {
    // known answers: K = 0, IV = 0, empty / one zero block (NIST GCM test cases 1, 2, 13, 14)
    const struct { int klen; int len; const char *ct, *tag; } kats[] = {
        {16, 0, "", "58e2fccefa7e3061367f1d57a4e7455a"},
        {16, 16, "0388dace60b6a392f328c2b971b2fe78", "ab6e47d42cec13bdf53a67b21257bddf"},
        {32, 0, "", "530f8afbc74536b9a963b4f1c4cb738b"},
        {32, 16, "cea7403d4d606b6e074ec5d3baf39d18", "d0d1c8a799996bf0265b98b5d48ab919"},
    };
    for (const auto &k : kats) {
        uint8_t key[32] = {0}, iv[12] = {0}, tag[16];
        std::vector<uint8_t> data((size_t)k.len, 0);
        CHECK(gcm(false, key, k.klen, iv, nullptr, 0, data.data(), data.size(), tag));
        CHECK(data == hex(k.ct));
        CHECK(memcmp(tag, hex(k.tag).data(), 16) == 0);
    }
    // round trips and forgeries over the odd lengths, exact-size buffers
    const int alens[] = {0, 8, 12, 16, 28, 33}, dlens[] = {0, 1, 15, 16, 17, 31, 32, 33, 1188};
    uint32_t x = 7714;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (uint8_t)(x >> 24); };
    for (int klen : {16, 32})
        for (int alen : alens)
            for (int dlen : dlens) {
                std::vector<uint8_t> key((size_t)klen), iv(12), aad((size_t)alen), pt((size_t)dlen), tag(16);
                for (auto *v : {&key, &iv, &aad, &pt})
                    for (auto &b : *v) b = rnd();
                std::vector<uint8_t> ct(pt);
                CHECK(gcm(false, key.data(), klen, iv.data(), aad.data(), aad.size(), ct.data(), ct.size(), tag.data()));
                if (dlen) CHECK(ct != pt);
                std::vector<uint8_t> back(ct), t2(tag);
                t2[rnd() & 15] ^= 1;
                CHECK(!gcm(true, key.data(), klen, iv.data(), aad.data(), aad.size(), back.data(), back.size(), t2.data()));
                CHECK(back == ct); // untouched on a mismatch
                CHECK(gcm(true, key.data(), klen, iv.data(), aad.data(), aad.size(), back.data(), back.size(), tag.data()));
                CHECK(back == pt);
            }
    // RFC 7714 11: the AES-CM PRF over the zero-padded 12-byte salt
    for (int klen : {16, 32})
        for (int rtcp = 0; rtcp < 2; rtcp++) {
            std::vector<uint8_t> mk((size_t)klen), ms(12), enc((size_t)klen), enc2((size_t)klen);
            for (auto &b : mk) b = rnd();
            for (auto &b : ms) b = rnd();
            uint8_t salt[14], salt2[14], auth[20], ms14[14] = {0};
            srtp::derive_session_keys_gcm(mk.data(), klen, ms.data(), rtcp != 0, enc.data(), salt);
            memcpy(ms14, ms.data(), 12);
            srtp::derive_session_keys_n(mk.data(), klen, ms14, rtcp != 0, enc2.data(), auth, salt2);
            CHECK(enc == enc2 && memcmp(salt, salt2, 12) == 0 && salt[12] == 0 && salt[13] == 0);
        }
    // the GPU batch's key block (srtp_aes_gcm_device): the key schedule and
    // table aes_gcm itself uses, nr, and zero everywhere else, written into
    // an exact-size heap object
    for (int klen : {16, 32}) {
        std::vector<uint8_t> key((size_t)klen);
        for (auto &b : key) b = rnd();
        std::vector<srtp::GcmKeyArg> ka(1);
        memset((void *)ka.data(), 0xff, sizeof(srtp::GcmKeyArg));
        srtp::gcm_key_arg(key.data(), klen, ka.data());
        uint32_t rk[60] = {0};
        uint64_t tab[16][2];
        uint8_t h[16] = {0};
        const int nr = srtp::aes_expand_le(key.data(), klen, rk);
        srtp::aes_encrypt_block_nr(rk, nr, h, h);
        srtp::gcm_htable(h, tab);
        CHECK(ka[0].nr == nr && nr == (klen == 16 ? 10 : 14));
        CHECK(memcmp(ka[0].rk, rk, sizeof rk) == 0);
        CHECK(memcmp(ka[0].htab, tab, sizeof tab) == 0);
        CHECK(ka[0].pad[0] == 0 && ka[0].pad[1] == 0 && ka[0].pad[2] == 0);
        // one multiplication by hand: (0 ^ x^0) * H = H, the table's entry 8
        uint8_t y[16] = {0}, one[16] = {0x80};
        srtp::gcm_mult_xor(ka[0].htab, y, one);
        CHECK(memcmp(y, h, 16) == 0);
    }
    // srtp_aes_gcm_device's argument rules (the key test comes before n == 0)
    {
        const uint8_t k[32] = {0};
        int x = 0;
        const void *p = &x;
        CHECK(srtp::gcm_batch_check(k, 16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, 0) == 1);
        CHECK(srtp::gcm_batch_check(k, 32, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, 0) == 1);
        CHECK(srtp::gcm_batch_check(k, 24, p, p, p, p, p, p, p, false, 0) == -1);
        CHECK(srtp::gcm_batch_check(k, 24, p, p, p, p, p, p, p, false, 1) == -1);
        CHECK(srtp::gcm_batch_check(nullptr, 16, p, p, p, p, p, p, p, false, 1) == -1);
        CHECK(srtp::gcm_batch_check(k, 16, p, p, p, p, p, p, nullptr, false, 1) == 0);
        CHECK(srtp::gcm_batch_check(k, 16, p, p, p, p, p, p, nullptr, true, 1) == -1);
        CHECK(srtp::gcm_batch_check(k, 32, p, p, p, p, p, p, p, true, 1u << 31) == 0);
        const void *a[6] = {p, p, p, p, p, p};
        for (int i = 0; i < 6; i++) {
            a[i] = nullptr;
            CHECK(srtp::gcm_batch_check(k, 16, a[0], a[1], a[2], a[3], a[4], a[5], p, true, 1) == -1);
            a[i] = p;
        }
    }
    printf(failures ? "gcm_host_check: %d failures\n" : "gcm_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
