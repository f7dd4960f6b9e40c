// fanout_fec_check.cpp -- stand-alone check of the FEC rule (libjitsi_amd/csrc/
// fec_job.h: fec_record_ok, fec_member_ok, fec_member_v2, fec_head_word,
// fec_src_piece / fec_src_word, fec_accumulate, fec_piece and fec_store_bytes,
// the text k_fanout_fec compiles), for a sanitizer build (no GPU, no Python).
// Every member lies in a heap buffer of exactly its length rounded up to 16 --
// what its region owns at the least -- with the bytes at and past its length
// set to junk, and is loaded the way the kernel loads it: the first two words
// through a reader that aborts outside [0, len), then for every output piece
// the aligned 16-byte piece and the aligned 4-byte word the rule names, so that
// AddressSanitizer sees any load outside the buffer.  The packet is rebuilt
// piece by piece into a heap buffer of exactly fec_store_bytes and compared
// with a separate byte-wise restatement of FECSender.FECPacket.addMedia and
// finish (transform/fec/FECSender.java:319-412) and of
// REDTransformEngine.transform (transform/REDTransformEngine.java:151-182) over
// Java byte arrays: counts 1..16, both modes, member lengths around every piece
// boundary the kernel has (12..17, 27..30, 43..45, 1008..1012, 2032..2036, 1200)
// alone and mixed, and destinations that fit, are one byte short and hold less
// than a piece.  The refusals of the record and of a member are swept too.
//
//   make -C tools fanout_fec_check      (built with -fsanitize=address,undefined)
//   tools/fanout_fec_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/fec_job.h"

using srtp::FanoutPiece;
using srtp::FecHead;
using srtp::FecWindow;

static int failures = 0;
static long packets = 0, pieces = 0, refusals = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static int up16(int v) { return (v + 15) & ~15; }
static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

struct Reader { // the member's len bytes; anything else ends the program
    const uint8_t *p;
    int len;
    int operator()(int i) const {
        if (i < 0 || i >= len) {
            printf("FAIL: the rule read index %d of %d\n", i, len);
            abort();
        }
        return p[i];
    }
};

// ---- the reference, restated over Java byte arrays
static Bytes reference(const std::vector<Bytes> &media, uint32_t ssrc, int pt, int red_pt) {
    Bytes buf(1500, 0); // FECTransformEngine.INITIAL_BUFFER_SIZE
    int base = -1, num = 0, plen = -1, last_seq = -1;
    uint8_t last_ts[4] = {0, 0, 0, 0};
    for (const Bytes &m : media) { // addMedia
        const int mpl = (int)m.size() - 12;
        if ((int)buf.size() < mpl + 12 + 14) buf.resize((size_t)mpl + 26, 0);
        if (base == -1) {
            base = (m[2] << 8) | m[3];
            for (int i = 0; i < 8; i++) buf[12 + (size_t)i] = m[(size_t)i];
            buf[20] = (uint8_t)(mpl >> 8 & 0xff);
            buf[21] = (uint8_t)(mpl & 0xff);
            for (int i = 0; i < mpl; i++) buf[26 + (size_t)i] = m[12 + (size_t)i];
        } else {
            for (int i = 0; i < 8; i++) buf[12 + (size_t)i] ^= m[(size_t)i];
            buf[20] ^= (uint8_t)(mpl >> 8 & 0xff);
            buf[21] ^= (uint8_t)(mpl & 0xff);
            for (int i = 0; i < mpl; i++) buf[26 + (size_t)i] ^= m[12 + (size_t)i];
        }
        last_seq = (m[2] << 8) | m[3];
        memcpy(last_ts, &m[4], 4);
        if (mpl > plen) plen = mpl;
        num++;
    }
    buf[0] = 0x80; // finish
    buf[1] = (uint8_t)((buf[1] & 0x80) | (pt & 0x7F));
    buf[2] = (uint8_t)((last_seq + 1) >> 8);
    buf[3] = (uint8_t)(last_seq + 1);
    buf[8] = (uint8_t)(ssrc >> 24);
    buf[9] = (uint8_t)(ssrc >> 16);
    buf[10] = (uint8_t)(ssrc >> 8);
    buf[11] = (uint8_t)ssrc;
    memcpy(&buf[4], last_ts, 4);
    buf[14] = (uint8_t)(base >> 8 & 0xff);
    buf[15] = (uint8_t)(base & 0xff);
    buf[22] = (uint8_t)(plen >> 8 & 0xff);
    buf[23] = (uint8_t)(plen & 0xff);
    const int mask = ((1 << num) - 1) << (16 - num);
    buf[24] = (uint8_t)(mask >> 8 & 0xff);
    buf[25] = (uint8_t)(mask & 0xff);
    buf.resize((size_t)26 + (size_t)plen);
    if (red_pt < 0) return buf;
    Bytes w(buf.size() + 1); // REDTransformEngine.transform: version 2, header length 12
    memcpy(&w[0], &buf[0], 12);
    memcpy(&w[13], &buf[12], buf.size() - 12);
    w[12] = (uint8_t)(buf[1] & 0x7F);
    w[1] = (uint8_t)((w[1] & 0x80) | red_pt);
    return w;
}

// ---- the rule, driven the way the kernel drives it
struct Member {
    uint8_t *region; // exactly up16(len) bytes on the heap
    int len;
};
static uint32_t load32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static void one(const std::vector<int> &lens, int mode, int dst_cap) {
    const int count = (int)lens.size();
    const uint32_t ssrc = rnd();
    const int pt = (int)(rnd() & 127), red_pt = (int)(rnd() & 127);
    std::vector<Member> mem;
    std::vector<Bytes> media;
    for (int len : lens) {
        Member m{(uint8_t *)malloc((size_t)up16(len)), len};
        for (int i = 0; i < up16(len); i++) m.region[i] = (uint8_t)rnd();
        m.region[0] = (uint8_t)(0x80 | (m.region[0] & 0x3F));
        mem.push_back(m);
        media.push_back(Bytes(m.region, m.region + len));
    }
    CHECK(srtp::fec_record_ok(0, (uint32_t)count, (uint32_t)pt, (uint32_t)red_pt, (uint32_t)mode, (uint32_t)count, -1));
    FecHead h{};
    for (int k = 0; k < count; k++) {
        const Reader rd{mem[(size_t)k].region, mem[(size_t)k].len};
        CHECK(srtp::fec_member_ok(0, 0, rd.len, rd.len));
        uint32_t w[2] = {0, 0};
        for (int i = 0; i < 8; i++) w[i / 4] |= (uint32_t)rd(i) << (8 * (i % 4));
        CHECK(srtp::fec_member_v2(w[0]));
        const int l = rd.len - 12;
        h.x0 ^= w[0];
        h.x1 ^= w[1];
        h.len_xor ^= l;
        h.plen = l > h.plen ? l : h.plen;
        if (k == 0) h.first_w0 = w[0];
        h.last_w0 = w[0];
        h.last_w1 = w[1];
    }
    h.count = count;
    h.mode = mode;
    h.ssrc = ssrc;
    h.pt = (uint32_t)pt;
    h.red_pt = (uint32_t)red_pt;
    const Bytes want = reference(media, ssrc, pt, mode == srtp::kFecRed ? red_pt : -1);
    const int len_out = srtp::fec_len_out(h);
    CHECK(len_out == (int)want.size());
    const int store = srtp::fec_store_bytes(len_out, dst_cap);
    CHECK(store == up16(len_out < dst_cap ? len_out : dst_cap) && store <= up16(dst_cap));
    uint8_t *out = (uint8_t *)malloc(store ? (size_t)store : 1);
    for (int q = 0; q < store / 16; q++) {
        FecWindow a{0, 0, 0, 0, 0};
        for (const Member &m : mem) {
            const uint8_t *P = m.region + 16 * srtp::fec_src_piece(q, m.len); // ASan: inside up16(len)
            const uint8_t *W = m.region + 4 * srtp::fec_src_word(q, m.len);
            CHECK(P + 16 <= m.region + up16(m.len) && W + 4 <= m.region + up16(m.len));
            srtp::fec_accumulate(a, FanoutPiece{load32(P), load32(P + 4), load32(P + 8), load32(P + 12)}, load32(W), q,
                                 m.len);
        }
        {
            const uint8_t *P = mem[0].region; // an empty batch slot: a piece 0 with len 0
            FecWindow b = a;
            srtp::fec_accumulate(b, FanoutPiece{load32(P), load32(P + 4), load32(P + 8), load32(P + 12)}, load32(P), q, 0);
            CHECK(memcmp(&a, &b, sizeof a) == 0);
        }
        const FanoutPiece o = srtp::fec_piece(a, q, h);
        memcpy(out + 16 * q, &o, 16);
        pieces++;
    }
    for (int i = 0; i < store; i++) { // the packet, and zeros from its end to the piece's
        const uint8_t w = i < len_out ? want[(size_t)i] : 0;
        if (out[i] != w) {
            CHECK(out[i] == w);
            if (failures < 20) printf("  count %d mode %d len_out %d byte %d: %02x, want %02x\n", count, mode, len_out, i, out[i], w);
            break;
        }
    }
    free(out);
    for (Member &m : mem) free(m.region);
    packets++;
}

static void refusals_sweep() {
    using namespace srtp;
    const uint32_t P = kFecPlain, R = kFecRed;
    CHECK(fec_record_ok(0, 1, 0, 0, P, 1, -1) && fec_record_ok(3, 16, 127, 255, P, 19, -1) &&
          fec_record_ok(3, 16, 127, 127, R, 19, -1));
    CHECK(!fec_record_ok(0, 0, 0, 0, P, 4, -1) && !fec_record_ok(0, 17, 0, 0, P, 40, -1));
    CHECK(!fec_record_ok(0, 4, 0, 0, P, 3, -1) && !fec_record_ok(2, 2, 0, 0, P, 3, -1) &&
          !fec_record_ok(0xFFFFFFFFu, 2, 0, 0, P, 0xFFFFFFFFu, -1) && !fec_record_ok(5, 1, 0, 0, P, 4, -1));
    CHECK(!fec_record_ok(0, 1, 128, 0, P, 1, -1) && !fec_record_ok(0, 1, 0, 128, R, 1, -1));
    CHECK(!fec_record_ok(0, 1, 0, 0, 0, 1, -1) && !fec_record_ok(0, 1, 0, 0, 3, 1, -1) && !fec_record_ok(0, 1, 0, 0, 255, 1, -1));
    CHECK(!fec_record_ok(0, 1, 0, 0, P, 1, 0) && !fec_record_ok(0, 1, 0, 0, P, 1, -2) && !fec_record_ok(0, 1, 0, 0, P, 1, 7));
    CHECK(fec_member_index_ok(0, 1) && fec_member_index_ok(6, 7) && !fec_member_index_ok(-1, 7) && !fec_member_index_ok(7, 7));
    CHECK(fec_member_ok(0, 0, 12, 12) && fec_member_ok(0x3u, 0, 65535, 65535));
    CHECK(!fec_member_ok(kFanFlagSkip, 0, 40, 40) && !fec_member_ok(0, 1, 40, 40) && !fec_member_ok(0, 2, 40, 40) &&
          !fec_member_ok(0, 0, 11, 40) && !fec_member_ok(0, 0, 0, 40) && !fec_member_ok(0, 0, -1, 40) &&
          !fec_member_ok(0, 0, 41, 40) && !fec_member_ok(0, 0, 40, -1) && !fec_member_ok(0, 0, 65536, 65536));
    CHECK(fec_member_v2(0x80) && fec_member_v2(0xFFFFFFBFu) && !fec_member_v2(0x40) && !fec_member_v2(0xC0) && !fec_member_v2(0));
    CHECK(fec_store_bytes(40, -1) == 0 && fec_store_bytes(-1, 40) == 0 && fec_store_bytes(65550, 70000) == 65536);
    refusals += 40;
}

int main() {
    refusals_sweep();
    const int single[] = {12, 13, 14, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1008, 1009, 1010, 1011, 1012, 1200,
                          2032, 2033, 2034, 2035, 2036};
    const int counts[] = {1, 2, 3, 15, 16};
    for (int mode = 1; mode <= 2; mode++) {
        for (int len : single)
            for (int count : counts) {
                const int len_out = len + 14 + (mode == 2);
                for (int cap : {len_out + 20, len_out, len_out - 1, 15, 0}) one(std::vector<int>((size_t)count, len), mode, cap);
            }
        for (int count = 1; count <= 16; count++) // every count, mixed lengths: the longest first, in the middle, last
            for (int where = 0; where < 3; where++)
                for (int rep = 0; rep < 12; rep++) {
                    std::vector<int> lens;
                    const int longest = single[rnd() % 24];
                    for (int k = 0; k < count; k++) lens.push_back(12 + (int)(rnd() % (uint32_t)(longest - 11)));
                    lens[(size_t)(where == 0 ? 0 : where == 1 ? count / 2 : count - 1)] = longest;
                    one(lens, mode, longest + 40);
                }
        one({65535}, mode, 65535); // the largest region: len_out past every cap
        one({12, 65535, 12}, mode, 65535);
    }
    printf("fanout_fec_check: %ld packets, %ld pieces, %ld refusal checks, %d failures\n", packets, pieces, refusals, failures);
    return failures ? 1 : 0;
}
