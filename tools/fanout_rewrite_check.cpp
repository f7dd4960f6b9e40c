// fanout_rewrite_check.cpp -- stand-alone check of the per-destination rewrite
// rule (libjitsi_amd/csrc/fanout_job.h: fanout_rewrite_applies and
// fanout_rewrite_words, the text k_fanout_rw compiles), for a sanitizer build
// (no GPU, no Python): sweeps fanout_check's source lengths and capacities
// around 0..32 and 1200, all 16 masks (and bits above them) and target values
// with every byte distinct; replays each copy 16 bytes at a time between heap
// buffers of exactly the two regions' rounded sizes, patching the first piece
// between its load and its store as the kernel does; and compares the result
// with a byte-wise restatement of RawPacket's four setters applied to a plain
// copy of c = min(src_len, src_cap, dst_cap) bytes, applied only when c >= 12.
// Nothing behind the copy may be written and the source must be unchanged;
// AddressSanitizer sees any byte outside either region.
//
//   make -C tools fanout_rewrite_check      (built with -fsanitize=address,undefined)
//   tools/fanout_rewrite_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/fanout_job.h"

using srtp::FanoutJob;
using srtp::FanoutWords;

static int failures = 0;
static long cases = 0, replayed = 0, patched = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

static uint8_t pattern[4096];
static int up16(int v) { return (v + 15) & ~15; }
static int imin(int a, int b) { return a < b ? a : b; }

struct Record {
    uint32_t mask, ssrc, timestamp;
    uint16_t seq;
    uint8_t pt, reserved;
};

// RawPacket.setPayloadType, setSequenceNumber, setTimestamp, setSSRC, byte by byte
static void setters(uint8_t *p, const Record &r) {
    if (r.mask & 0x8u) p[1] = (uint8_t)((p[1] & 0x80) | (r.pt & 0x7F));
    if (r.mask & 0x2u) {
        p[2] = (uint8_t)(r.seq >> 8);
        p[3] = (uint8_t)r.seq;
    }
    if (r.mask & 0x4u)
        for (int i = 0; i < 4; i++) p[4 + i] = (uint8_t)(r.timestamp >> (24 - 8 * i));
    if (r.mask & 0x1u)
        for (int i = 0; i < 4; i++) p[8 + i] = (uint8_t)(r.ssrc >> (24 - 8 * i));
}

static uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void put_le32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

static void one(int L, int sc, int dc, uint32_t fl, int st, const Record &r, int byte1) {
    cases++;
    const FanoutJob j = srtp::fanout_job(0, 1, L, sc, st, dc, fl);
    const bool skipped = st != 0 || (fl & srtp::kFanFlagSkip);
    const int c = imin(L, imin(sc, dc));
    const bool want = !skipped && (r.mask & 0xFu) != 0 && c >= 12;
    const bool applies = srtp::fanout_rewrite_applies(j, L, sc, dc, r.mask);
    CHECK(applies == want);
    if (applies) CHECK(j.copy_bytes >= 16); // the patched piece is one the copy writes
    std::vector<uint8_t> src((size_t)up16(sc)), dst((size_t)up16(dc));
    uint8_t *sp = src.data(), *dp = dst.data();
    if (!src.empty()) {
        memcpy(sp, pattern, src.size());
        sp[1] = (uint8_t)byte1; // the marker bit setPayloadType keeps
    }
    const std::vector<uint8_t> before(src);
    if (!dst.empty()) memset(dp, 0xEE, dst.size());
    // the copy as k_fanout_rw makes it: a piece is loaded, the first one patched, then stored
    for (int o = 0; o < j.copy_bytes; o += 16) {
        uint8_t piece[16];
        memcpy(piece, sp + o, 16);
        if (o == 0 && applies) {
            const FanoutWords w = srtp::fanout_rewrite_words(le32(piece), le32(piece + 4), le32(piece + 8), r.mask,
                                                             r.ssrc, r.timestamp, r.seq, r.pt);
            put_le32(piece, w.w0);
            put_le32(piece + 4, w.w1);
            put_le32(piece + 8, w.w2);
            patched++;
        }
        memcpy(dp + o, piece, 16);
    }
    CHECK(src == before);
    if (skipped) CHECK(j.copy_bytes == 0);
    // the restatement: a plain copy of c bytes, the setters applied when the fixed header is there
    if (!skipped && c > 0) {
        std::vector<uint8_t> ref(before.begin(), before.begin() + c);
        if (c >= 12) setters(ref.data(), r);
        CHECK(memcmp(dp, ref.data(), (size_t)c) == 0);
        // the bytes of the last piece past c are the source's, as without records
        CHECK(memcmp(dp + c, before.data() + c, (size_t)(j.copy_bytes - c)) == 0);
    }
    for (int i = j.copy_bytes; i < (int)dst.size(); i++) // nothing behind the copy
        if (dp[i] != 0xEE) {
            CHECK(dp[i] == 0xEE);
            break;
        }
    replayed++;
}

int main() {
    for (size_t i = 0; i < sizeof pattern; i++) pattern[i] = (uint8_t)(i * 7 + 3);
    std::vector<int> lens, caps;
    for (int L = 0; L <= 32; L++) lens.push_back(L);
    for (int d = -17; d <= 17; d++) lens.push_back(1200 + d);
    for (int c : {0, 16, 32, 1200, 1216})
        for (int d : {-17, -16, -5, -4, -1, 0, 1, 16})
            if (c + d >= 0) caps.push_back(c + d);
    for (int c = 8; c <= 13; c++) caps.push_back(c);
    // target values with every byte distinct, and the all-ones / all-zeros ends
    const Record values[] = {{0, 0x11223344u, 0x55667788u, 0x99AAu, 0xBB, 0xCC},
                             {0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFu, 0xFF, 0xFF},
                             {0, 0u, 0u, 0u, 0, 0}};
    for (int L : lens)
        for (int sc : caps)
            for (int dc : caps)
                for (uint32_t mask = 0; mask < 16; mask++) {
                    Record r = values[(L + mask) % 3];
                    r.mask = mask;
                    one(L, sc, dc, 0u, 0, r, (L & 1) ? 0xE0 : 0x60);
                }
    // skipped entries, mask bits above 0xF, and a payload type with its top bit set
    for (int L : {0, 11, 12, 16, 1200})
        for (int c : {0, 11, 12, 16, 1216})
            for (uint32_t mask : {0x0u, 0xFu, 0x10u, 0x1Fu, 0xFFFFFFF0u, 0xFFFFFFFFu, 0x80000001u})
                for (uint32_t fl : {0u, 0x2u, srtp::kFanFlagSkip, srtp::kFanFlagSkip | 0x4u})
                    for (int st : {0, 2, 9}) {
                        Record r = values[0];
                        r.mask = mask;
                        one(L, c, c, fl, st, r, 0x80);
                    }
    // the words alone: each field lands where its setter puts it, and nowhere else
    {
        const uint8_t h[12] = {0x80, 0xE0, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A};
        const FanoutWords w = srtp::fanout_rewrite_words(le32(h), le32(h + 4), le32(h + 8), 0xFu, 0x11223344u,
                                                         0x55667788u, 0x99AAu, 0xBBu);
        uint8_t g[12];
        put_le32(g, w.w0);
        put_le32(g + 4, w.w1);
        put_le32(g + 8, w.w2);
        const uint8_t want[12] = {0x80, 0x80 | 0x3B, 0x99, 0xAA, 0x55, 0x66, 0x77, 0x88, 0x11, 0x22, 0x33, 0x44};
        CHECK(memcmp(g, want, 12) == 0);
    }
    printf("fanout_rewrite_check: %ld cases, %ld copies replayed, %ld patched, %d failures\n", cases, replayed,
           patched, failures);
    return failures || patched == 0 ? 1 : 0;
}
