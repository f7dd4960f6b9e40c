// fanout_pay_check.cpp -- stand-alone check of the payload-patch rule
// (libjitsi_amd/csrc/fanout_job.h: fanout_pay_bound, fanout_pay_on,
// fanout_pay_piece and fanout_pay_byte, the text k_fanout_pay compiles), for a
// sanitizer build (no GPU, no Python).  It sweeps c = min(src_len, src_cap,
// dst_cap) over 12..40 and over 1008..1040 and 2032..2064 (the piece 63/64 and
// piece 127/128 boundaries of the copy loop: lane 63's first load against lane
// 0's second, the first trip against the second), reached through the source's
// length, the source's capacity and a truncating destination; both offsets over
// 0, 11, 12, c - 2, c - 1, c, c + 1 and every straddle of a 16-byte boundary in
// range; overlapping and equal offsets; skipped entries and negative lengths.
// Every copy is replayed 16 bytes at a time through fanout_pay_piece -- patch
// 0, then patch 1, under the kernel's predicate -- between heap buffers of
// exactly the two regions' rounded sizes, and compared with a separate
// byte-wise restatement of the reference's writes (RawPacket.writeShort,
// RawPacket.java:1334-1337; rewriteFEC's two stores,
// ExtendedSequenceNumberInterval.java:383-384) on a buffer of exactly c bytes.
// No byte outside [12, c) may differ from the plain copy, nothing behind the
// copy may be written and the source must be unchanged; AddressSanitizer sees
// any byte outside either region.
//
//   make -C tools fanout_pay_check      (built with -fsanitize=address,undefined)
//   tools/fanout_pay_check
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../libjitsi_amd/csrc/fanout_job.h"

using srtp::FanoutJob;
using srtp::FanoutPiece;

static int failures = 0;
static long cases = 0, replayed = 0, patched = 0, halves = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static int up16(int v) { return (v + 15) & ~15; }
static int imin(int a, int b) { return a < b ? a : b; }

struct Record { // srtp_fanout_payload
    uint16_t at0;
    uint8_t b0[2];
    uint16_t at1;
    uint8_t b1[2];
};

// ---- the reference, restated byte by byte over a buffer of exactly the copied bytes.  A write
// at or past the end is the one the rule leaves out (Java would throw: the rule is per byte).
static void write_byte(Bytes &buf, int i, uint8_t v) {
    if (i < (int)buf.size()) buf[(size_t)i] = v;
}
static void reference(Bytes &buf, const Record &r) {
    if (r.at0 >= 12) { // below byte 12 a patch is refused whole
        write_byte(buf, r.at0, r.b0[0]);
        write_byte(buf, r.at0 + 1, r.b0[1]);
    }
    if (r.at1 >= 12) {
        write_byte(buf, r.at1, r.b1[0]);
        write_byte(buf, r.at1 + 1, r.b1[1]);
    }
}

static uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void put_le32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}
static FanoutPiece load(const uint8_t *p) { return FanoutPiece{le32(p), le32(p + 4), le32(p + 8), le32(p + 12)}; }
static bool same(const FanoutPiece &a, const FanoutPiece &b) {
    return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3;
}

// one patch over the piece, as the kernel's store side has it
static FanoutPiece paid(const FanoutPiece &p, int q, int at, uint32_t v0, uint32_t v1, int c) {
    const bool on = srtp::fanout_pay_on(at, c);
    const FanoutPiece o = srtp::fanout_pay_piece(p, q, at, v0, v1, c);
    const bool hit = on && (q == (at >> 4) || q == ((at + 1) >> 4));
    if (!hit) CHECK(same(o, p)); // outside the predicate the function changes nothing either
    return hit ? o : p;
}

static void one(int L, int sc, int dc, uint32_t fl, int st, const Record &r) {
    cases++;
    const FanoutJob j = srtp::fanout_job(0, 1, L, sc, st, dc, fl);
    const bool skipped = st != 0 || (fl & srtp::kFanFlagSkip);
    const int c = srtp::fanout_pay_bound(j, L, sc, dc);
    const int plain = skipped || L < 0 || sc < 0 || dc < 0 ? 0 : imin(imin(L, 65535), imin(sc, dc));
    CHECK(c == plain);
    CHECK(c <= j.copy_bytes);
    Bytes src((size_t)up16(sc < 0 ? 0 : sc)), dst((size_t)up16(dc < 0 ? 0 : dc));
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i * 7 + 3);
    const Bytes before(src);
    uint8_t *dp = dst.data();
    if (!dst.empty()) memset(dp, 0xEE, dst.size());
    CHECK((size_t)j.copy_bytes <= src.size() && (size_t)j.copy_bytes <= dst.size());
    for (int o = 0; o < j.copy_bytes; o += 16) {
        const int q = o / 16;
        FanoutPiece p = load(src.data() + o);
        p = paid(p, q, r.at0, r.b0[0], r.b0[1], c);
        p = paid(p, q, r.at1, r.b1[0], r.b1[1], c);
        uint8_t piece[16];
        put_le32(piece, p.w0);
        put_le32(piece + 4, p.w1);
        put_le32(piece + 8, p.w2);
        put_le32(piece + 12, p.w3);
        memcpy(dp + o, piece, 16);
    }
    CHECK(src == before);
    if (skipped) CHECK(j.copy_bytes == 0 && c == 0);
    if (c > 0) {
        Bytes ref(before.begin(), before.begin() + c);
        reference(ref, r);
        CHECK(memcmp(dp, ref.data(), (size_t)c) == 0);
        for (int i = 0; i < c; i++) { // what the abs-send-time walk would read of the copy
            const int b = srtp::fanout_pay_byte(
                srtp::fanout_pay_byte(before[(size_t)i], i, r.at0, r.b0[0], r.b0[1], c), i, r.at1, r.b1[0], r.b1[1], c);
            if (b != dp[i]) {
                CHECK(b == dp[i]);
                break;
            }
        }
        if (memcmp(ref.data(), before.data(), (size_t)c) != 0) patched++;
        if ((r.at0 >= 12 && r.at0 == c - 1) || (r.at1 >= 12 && r.at1 == c - 1)) halves++;
    }
    // no byte outside [12, c) differs from the plain copy: the header, and the last piece's tail
    for (int i = 0; i < j.copy_bytes; i++)
        if ((i < 12 || i >= c) && dp[i] != before[(size_t)i]) {
            CHECK(dp[i] == before[(size_t)i]);
            break;
        }
    for (int i = j.copy_bytes; i < (int)dst.size(); i++) // nothing behind the copy
        if (dp[i] != 0xEE) {
            CHECK(dp[i] == 0xEE);
            break;
        }
    replayed++;
}

static Record rec(int at0, int at1) {
    Record r = {(uint16_t)at0, {0xC1, 0xD2}, (uint16_t)at1, {0xE3, 0xF4}};
    return r;
}

static std::set<int> small_set(int c) {
    std::set<int> s = {0, 11, 12};
    for (int d = -2; d <= 1; d++)
        if (c + d >= 0) s.insert(c + d);
    return s;
}

static void sweep(int c) {
    const std::set<int> few = small_set(c);
    std::set<int> all(few);
    for (int b = 16; b <= c + 16; b += 16) { // every straddle of a 16-byte boundary in range, and the byte behind it
        all.insert(b - 1);
        all.insert(b);
    }
    for (int at0 : all) {
        std::set<int> other(few);
        for (int d = -2; d <= 2; d++) // overlapping and equal offsets
            if (at0 + d >= 0) other.insert(at0 + d);
        for (int at1 : other) {
            one(c, c + 40, c + 40, 0u, 0, rec(at0, at1)); // the packet ends there
            if (few.count(at0)) {
                one(c + 40, c + 40, c, 0u, 0, rec(at0, at1)); // the destination does
                one(c + 40, c, c + 40, 0u, 0, rec(at0, at1)); // the source region does
            }
        }
    }
    for (int at : few) {
        one(c, c, c, srtp::kFanFlagSkip, 0, rec(at, at));
        one(c, c, c, 0u, 2, rec(at, 12));
        one(-1, c, c, 0u, 0, rec(12, at));
        one(c, -1, c, 0u, 0, rec(12, at));
        one(c, c, -1, 0u, 0, rec(12, at));
        one(0x7FFFFFFF, c, c + 16, 0u, 0, rec(at, c - 1));
    }
}

int main() {
    for (int c = 0; c <= 40; c++) sweep(c);
    for (int c = 1008; c <= 1040; c++) sweep(c);
    for (int c = 2032; c <= 2064; c++) sweep(c);
    // the largest region: offsets at the top of the 16-bit range
    for (int at : {65519, 65533, 65534, 65535}) {
        one(65535, 65535, 65535, 0u, 0, rec(at, 12));
        one(70000, 65535, 65535, 0u, 0, rec(12, at));
        one(65534, 65535, 65535, 0u, 0, rec(at, at));
    }
    // all-zero and values: every byte value once, both patches in one piece and in one word
    one(100, 100, 100, 0u, 0, rec(0, 0));
    for (int v = 0; v < 256; v++) {
        Record r = {(uint16_t)(16 + v % 14), {(uint8_t)v, (uint8_t)(255 - v)}, (uint16_t)(17 + v % 13), {(uint8_t)(v * 3), (uint8_t)(v ^ 0x5A)}};
        one(64, 64, 64, 0u, 0, r);
    }
    printf("fanout_pay_check: %ld cases, %ld copies replayed, %ld patched, %ld half patches, %d failures\n", cases,
           replayed, patched, halves, failures);
    return failures || patched == 0 || halves == 0 ? 1 : 0;
}
