// gcm_pow_check.cpp -- stand-alone check, for a sanitizer build (no GPU, no
// Python), of the host code the wave-per-packet GCM kernels rest on: the
// general GF(2^128) product against the table multiplication, the chain of
// powers of H, a GHASH summed from powers in chunks of 64 against the serial
// one, and the per-packet paths' trailer room.
//
//   make -C tools gcm_pow_check      (built with -fsanitize=address,undefined)
//   tools/gcm_pow_check
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/gcm_job.h"
#include "../libjitsi_amd/csrc/host_crypto.h"

static int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);      \
            failures++;                                              \
        }                                                            \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}

static void to_bytes(const uint64_t v[2], uint8_t out[16]) { // {low, high} halves -> the 16 block bytes
    for (int i = 0; i < 8; i++) {
        out[i] = (uint8_t)(v[1] >> (56 - 8 * i));
        out[8 + i] = (uint8_t)(v[0] >> (56 - 8 * i));
    }
}

int main() {
    using namespace srtp;
    for (int round = 0; round < 64; round++) {
        uint64_t H[2] = {rnd(), rnd()};
        if (round == 0) H[0] = 0, H[1] = 0x8000000000000000ull; // the field's 1
        if (round == 1) H[0] = H[1] = ~0ull;
        uint8_t hb[16];
        to_bytes(H, hb);
        uint64_t tab[16][2];
        gcm_htable(hb, tab);
        // gf128_mul(x, H) against the table multiplication
        for (int t = 0; t < 200; t++) {
            uint64_t x[2] = {rnd(), rnd()};
            if (t == 0) x[0] = x[1] = 0;
            if (t == 1) x[0] = x[1] = ~0ull;
            if (t == 2) x[0] = 1, x[1] = 0;
            uint8_t y[16] = {0}, xb[16], zb[16];
            uint64_t z[2], z2[2];
            to_bytes(x, xb);
            gcm_mult_xor(tab, y, xb);
            gf128_mul(x, H, z);
            to_bytes(z, zb);
            CHECK(memcmp(y, zb, 16) == 0);
            gf128_mul(H, x, z2); // the field is commutative
            CHECK(z[0] == z2[0] && z[1] == z2[1]);
        }
        // the power chain: pw[k] = pw[k - 1] * H, by the table
        uint64_t pw[kGcmPowers][2];
        gcm_hpowers(hb, pw);
        CHECK(pw[0][0] == H[0] && pw[0][1] == H[1]);
        uint8_t y[16] = {0};
        to_bytes(H, y);
        const uint8_t zero[16] = {0};
        for (int k = 1; k < kGcmPowers; k++) {
            uint8_t pb[16];
            gcm_mult_xor(tab, y, zero);
            to_bytes(pw[k], pb);
            CHECK(memcmp(y, pb, 16) == 0);
        }
        // GHASH from powers, 64 blocks at a time, against the serial chain
        for (int T : {1, 2, 63, 64, 65, 77, 128, 129}) {
            std::vector<uint64_t> X(2 * (size_t)T);
            for (auto &v : X) v = rnd();
            uint8_t ys[16] = {0};
            for (int i = 0; i < T; i++) {
                uint8_t xb[16];
                to_bytes(&X[2 * (size_t)i], xb);
                gcm_mult_xor(tab, ys, xb);
            }
            uint64_t Z[2] = {0, 0};
            for (int base = 0; base < T; base += kGcmPowers) {
                const int m = T - base < kGcmPowers ? T - base : kGcmPowers;
                uint64_t acc[2] = {0, 0};
                for (int l = 0; l < m; l++) {
                    uint64_t x[2] = {X[2 * (size_t)(base + l)], X[2 * (size_t)(base + l) + 1]}, p[2];
                    if (l == 0) x[0] ^= Z[0], x[1] ^= Z[1];
                    gf128_mul(x, pw[m - l - 1], p);
                    acc[0] ^= p[0];
                    acc[1] ^= p[1];
                }
                Z[0] = acc[0];
                Z[1] = acc[1];
            }
            uint8_t zb[16];
            to_bytes(Z, zb);
            CHECK(memcmp(ys, zb, 16) == 0);
        }
    }
    // gcm_key_arg_pow: the same key block as gcm_key_arg, and H's powers
    {
        uint8_t key[32];
        for (auto &b : key) b = (uint8_t)rnd();
        for (int klen : {16, 32}) {
            GcmKeyArg a, b;
            uint64_t pw[kGcmPowers][2], pw2[kGcmPowers][2];
            gcm_key_arg(key, klen, &a);
            gcm_key_arg_pow(key, klen, &b, pw);
            CHECK(memcmp(&a, &b, sizeof a) == 0);
            CHECK(pw[0][0] == a.htab[8][0] && pw[0][1] == a.htab[8][1]); // entry 8 is H itself
            uint8_t hb[16];
            to_bytes(pw[0], hb);
            gcm_hpowers(hb, pw2);
            CHECK(memcmp(pw, pw2, sizeof pw) == 0);
        }
    }
    // the trailer room: 16, or 20 for any non-zero switch value
    CHECK(trailer_room(0) == 16u);
    for (long long v = INT_MIN; v <= INT_MAX; v += 65537) CHECK(trailer_room((int)v) == (v ? 20u : 16u));
    for (int v : {INT_MIN, -1, 1, 2, 255, 256, INT_MAX}) CHECK(trailer_room(v) == 20u);
    // ... and it is what GCM SRTCP protect appends, SRTP's 16 fitting inside
    {
        const GcmJob c = gcm_packet_job(1, 0, 200, 200 + (int)trailer_room(1), 0, 0u, 1);
        CHECK(c.status == kGcmNoStatus && c.new_len == 200 + (int)trailer_room(1));
        CHECK(gcm_packet_job(1, 0, 200, 200 + (int)trailer_room(1) - 1, 0, 0u, 1).status == kGcmStCapacity);
        CHECK(gcm_packet_job(1, 0, 200, 200 + (int)trailer_room(0), 0, 0u, 1).status == kGcmStCapacity);
        CHECK(gcm_packet_job(0, 0, 200, 200 + (int)trailer_room(0), 12, 0u, 1).status == kGcmNoStatus);
    }
    printf(failures ? "gcm_pow_check: %d FAILED\n" : "gcm_pow_check: ok\n", failures);
    return failures ? 1 : 0;
}
