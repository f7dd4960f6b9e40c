// host_crypto.h -- control-plane crypto on the host: AES-128 key schedule and
// single-block encrypt (for the RFC 3711 4.3 key derivation PRF) and the SHA-1
// compression function (for the HMAC ipad/opad midstates).  Runs once per
// factory; the per-packet path is on the GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "srtp_types.h"

namespace srtp {

// Expanded AES-128 encryption key, 44 words.  Word i holds round-key bytes
// 4i..4i+3 in little-endian order (byte 4i in bits 0..7), the layout the
// gfx950 T-table rounds use.
void aes128_expand_le(const uint8_t key[16], uint32_t rk_le[44]);
// AES-128 (key_len 16) or AES-256 (32) key expansion in the same layout;
// returns the number of rounds (10 / 14), 4 * (nr + 1) words written.
int aes_expand_le(const uint8_t *key, int key_len, uint32_t rk_le[60]);
void aes_encrypt_block_nr(const uint32_t *rk_le, int nr, const uint8_t in[16], uint8_t out[16]);
void aes128_encrypt_block(const uint32_t rk_le[44], const uint8_t in[16], uint8_t out[16]);
// SHA-1 compression of one 64-byte block into state[5].
void sha1_compress(uint32_t state[5], const uint8_t block[64]);
extern const uint32_t kSha1Init[5];
// The AES forward T-table used by the device (LE layout: 2s | s<<8 | s<<16 | 3s<<24).
void aes_te0_le(uint32_t te0[256]);

// RFC 3711 4.3 key derivation exactly as SRTPCryptoContext.deriveSrtpKeys
// (labels 0,1,2; :393-447) or SRTCPCryptoContext.deriveSrtcpKeys (3,4,5;
// :158-211) with kdr == 0.
void derive_session_keys(const uint8_t master_key[16], const uint8_t master_salt[14], bool rtcp,
                         uint8_t enc[16], uint8_t auth[20], uint8_t salt[14]);
// The same with a 16- or 32-byte master key: the PRF is AES-128 / AES-256 and
// the session encryption key is key_len bytes (RFC 6188 4.1 for AES-256).
void derive_session_keys_n(const uint8_t *mk, int key_len, const uint8_t ms[14], bool rtcp,
                           uint8_t *enc, uint8_t auth[20], uint8_t salt[14]);
// With the Twofish PRF (twofish = true: the ZRTP Twofish policies key their
// TwofishEngine with the master key).
// auth_len: the policy's auth key length (20 for HMAC-SHA1, 32 for ZRTP's Skein).
void derive_session_keys_cipher(bool twofish, const uint8_t *mk, int key_len, const uint8_t ms[14],
                                bool rtcp, uint8_t *enc, uint8_t *auth, uint8_t salt[14],
                                int auth_len = 20);
// Twofish key schedule (key_len 16, 24 or 32): subkeys K[40] and the four g()
// tables (key-dependent S-boxes times the MDS columns); one block.
void twofish_schedule(const uint8_t *key, int key_len, uint32_t K[40], uint32_t T[4][256]);
void twofish_encrypt_block(const uint32_t K[40], const uint32_t T[4][256], const uint8_t in[16],
                           uint8_t out[16]);
// HMAC-SHA1 ipad/opad midstates for a 20-byte key.
void hmac_sha1_midstates(const uint8_t key[20], uint32_t ipad[5], uint32_t opad[5]);

// Skein-512 (version 1.3): UBI block types, and the key-schedule parity
// constant C240 of Threefish.
constexpr uint64_t kSkeinParity = 0x1BD11BDAA9FC1A22ull;
constexpr uint64_t kSkeinTypeKey = 0, kSkeinTypeCfg = 4, kSkeinTypeMsg = 48, kSkeinTypeOut = 63;
// The chaining value of a keyed Skein-512 with out_bits output bits after the
// key UBI (skipped for key_len 0) and the config UBI: SkeinMac's state before
// the first message byte.
void skein512_key_state(const uint8_t *key, int key_len, int out_bits, uint64_t g0[8]);
// Whole Skein-512 MAC (key_len 0: the plain hash), ceil(out_bits / 8) bytes.
void skein512_mac(const uint8_t *key, int key_len, int out_bits, const uint8_t *msg, size_t n,
                  uint8_t *out);


// AES-GCM (NIST SP 800-38D) with a 96-bit IV, as RFC 7714 uses it.  GHASH is
// Shoup's 4-bit table method: tab[i] = {low, high} 64-bit halves (big-endian
// bit order of the field element) of the 4-bit polynomial i times H, the table
// the gfx950 kernel multiplies with (GcmKeys::htab).
void gcm_htable(const uint8_t h[16], uint64_t tab[16][2]);
// y = (y ^ x) * H with that table (y, x: 16 bytes).
void gcm_mult_xor(const uint64_t tab[16][2], uint8_t y[16], const uint8_t x[16]);
// The general product a * b in GF(2^128) (SP 800-38D algorithm 1), elements as
// {low, high} halves in the bit order gcm_htable's entries have.
void gf128_mul(const uint64_t a[2], const uint64_t b[2], uint64_t out[2]);
// out[k] = H^(k + 1), k = 0..63, as such halves: with them GHASH is the
// polynomial sum X_1 H^T + ... + X_T H^1, 64 terms at a time (k_gcm_wave;
// GcmPow, GcmBatchWave::pow).
constexpr int kGcmPowers = 64;
void gcm_hpowers(const uint8_t h[16], uint64_t out[kGcmPowers][2]);
// Seal (open = false) or open data[0, len) in place under the expanded key
// rk / nr; tag[16] is written (seal) or compared (open: returns false on a
// mismatch and leaves data untouched).
bool aes_gcm(bool open, const uint32_t *rk_le, int nr, const uint8_t iv[12], const uint8_t *aad,
             size_t aad_len, uint8_t *data, size_t len, uint8_t tag[16]);
// The key block of the stateless GPU batch (srtp_aes_gcm_device): the expanded
// key (key_len 16 or 32) and gcm_htable(E_K(0^128)); every other byte zero.
void gcm_key_arg(const uint8_t *key, int key_len, GcmKeyArg *out);
// ... and with it gcm_hpowers(E_K(0^128)), for the wave-per-packet batch.
void gcm_key_arg_pow(const uint8_t *key, int key_len, GcmKeyArg *out, uint64_t pow[kGcmPowers][2]);
// The argument rules of srtp_aes_gcm_device after its engine test: -1 for a
// missing key or a key_len other than 16 / 32 (whatever n is); else 1 for
// n == 0 (nothing to launch, the arrays are not looked at); else -1 when an
// array is NULL (result only matters to open); else 0: launch.
int gcm_batch_check(const void *key, int key_len, const void *seg, const void *off, const void *aad_len,
                    const void *len, const void *iv, const void *tag, const void *result, bool open,
                    uint32_t n);
// RFC 7714 11: the session encryption key (key_len bytes) and the 12-byte
// session salt (salt[12..13] = 0) from a 12-byte master salt, by the AES-CM
// PRF of the key's size; no auth key.
void derive_session_keys_gcm(const uint8_t *mk, int key_len, const uint8_t ms[12], bool rtcp,
                             uint8_t *enc, uint8_t salt[14]);

} // namespace srtp
