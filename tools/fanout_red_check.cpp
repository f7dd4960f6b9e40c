// fanout_red_check.cpp -- stand-alone check of the RED rule (libjitsi_amd/csrc/
// red_job.h: red_wanted, red_rule, red_job, red_piece and red_byte, the text
// k_fanout_red compiles), for a sanitizer build (no GPU, no Python).  It drives
// the rule through a reader that aborts on any index outside [0, c) over every
// c in 12..96, CC 0..2, X on and off, both extension-length bytes from {0, 1, 2,
// 0x7F, 0x80, 0xFF} (and the lengths that bring the header's end to 0, 4 and 8),
// every value of the byte at the header's end and both modes, against a
// separate byte-wise restatement of REDFilterTransformEngine.transform
// (transform/REDFilterTransformEngine.java:95-145) and
// REDTransformEngine.transform (transform/REDTransformEngine.java:151-182) with
// Java's exceptions as a result code.  Every stripped or wrapped packet is then
// rebuilt 16 bytes at a time through red_piece -- the loads the kernel issues,
// clamped by red_src_piece / red_src_word -- between heap buffers of exactly the
// two regions' rounded sizes, so that AddressSanitizer sees any byte outside
// either, and compared with the restatement for every piece q; red_byte is held
// to the same bytes.
//
//   make -C tools fanout_red_check      (built with -fsanitize=address,undefined)
//   tools/fanout_red_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/red_job.h"

using srtp::FanoutJob;
using srtp::FanoutPiece;
using srtp::RedPlan;

static int failures = 0;
static long cases = 0, stripped = 0, wrapped = 0, dropped = 0, untouched = 0, pieces = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static int up16(int v) { return (v + 15) & ~15; }

struct Reader { // the packet's c bytes; anything else ends the program
    const uint8_t *p;
    int c;
    int operator()(int i) const {
        if (i < 0 || i >= c) {
            printf("FAIL: the rule read index %d of %d\n", i, c);
            abort();
        }
        return p[i];
    }
};

// ---- the reference, restated over a Java byte[] of exactly c bytes: -1 is an exception
static int sb(uint8_t v) { return v >= 128 ? (int)v - 256 : (int)v; }
static bool header_length(const Bytes &b, int *h) { // false: ArrayIndexOutOfBounds
    const int c = (int)b.size();
    *h = 12 + 4 * (b[0] & 15);
    if (b[0] & 0x10) {
        const int i = *h + 2;
        if (i >= c || i + 1 >= c) return false;
        *h += 4 + (sb(b[(size_t)i]) * 256 + b[(size_t)i + 1]) * 4; // (signed << 8) | unsigned, without the shift
    }
    return true;
}
static int reference(const Bytes &b, int mode, int red_pt, Bytes *out) {
    const int c = (int)b.size();
    *out = b;
    if ((b[0] >> 6) != 2) return 0;
    int h;
    if (mode == srtp::kRedStrip) {
        if (b[1] >= 200 && b[1] <= 211) return 0;
        if ((b[1] & 0x7F) != red_pt) return 0;
        if (!header_length(b, &h)) return -1;
        // isMultiBlock: false when the offset is outside the buffer
        const bool multi = h >= 0 && h < c && (b[(size_t)h] & 0x80);
        if (multi) return -1; // the iterator hands back offset -1 or walks off the buffer: arraycopy throws
        if (h < 0 || c - h < 0) return 0; // the guards: no primary block
        if (h >= c) return -1;            // buffer[offset]
        const uint8_t pt = b[(size_t)h] & 0x7F;
        out->clear();
        for (int i = 0; i < h; i++) out->push_back(b[(size_t)i]);
        for (int i = h + 1; i < c; i++) out->push_back(b[(size_t)i]);
        (*out)[1] = (uint8_t)((b[1] & 0x80) | pt); // h >= 4 here: h == 0 has bit 7 of b[0] set
        return 1;
    }
    if (!header_length(b, &h)) return -1;
    if (h < 0 || h > c) return -1; // arraycopy
    Bytes n((size_t)c + 1);
    for (int i = 0; i < h; i++) n[(size_t)i] = b[(size_t)i];
    for (int i = h; i < c; i++) n[(size_t)i + 1] = b[(size_t)i];
    n[(size_t)h] = b[1] & 0x7F;
    n[1] = (uint8_t)((n[1] & 0x80) | red_pt); // setPayloadType on the new buffer
    *out = n;
    return 2;
}

static uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void put_le32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

static void one(const Bytes &pkt, int mode, int red_pt, int src_cap, int dst_cap) {
    cases++;
    const int c = (int)pkt.size();
    const FanoutJob j = srtp::fanout_job(0, 1, c, src_cap, 0, dst_cap, 0u);
    const int want = srtp::red_wanted(j, c, src_cap, dst_cap, (uint32_t)mode, (uint32_t)red_pt, 0u);
    CHECK(want == (c <= src_cap && c <= dst_cap ? c : 0));
    if (!want) return;
    const Reader rd{pkt.data(), c};
    const RedPlan p = srtp::red_rule(rd, c, mode, red_pt);
    Bytes ref;
    const int r = reference(pkt, mode, red_pt, &ref);
    CHECK(p.result == r);
    if (p.result != r) return;
    const FanoutJob nj = srtp::red_job(j, p, dst_cap);
    if (r == 0) {
        untouched++;
        CHECK(p.shift == 0 && nj.copy_bytes == j.copy_bytes && nj.len_out == j.len_out && nj.flags_out == j.flags_out);
        return;
    }
    if (r < 0) {
        dropped++;
        CHECK(nj.copy_bytes == 0 && nj.len_out == 0 && (nj.flags_out & srtp::kFanFlagSkip));
        return;
    }
    (r == 1 ? stripped : wrapped)++;
    CHECK(p.shift == (r == 1 ? -1 : 1) && p.len_out == c + p.shift && p.len_out == (int)ref.size());
    CHECK(p.h >= 0 && p.h <= c && p.h % 4 == 0 && nj.len_out == p.len_out);
    CHECK(srtp::red_src_len(p, c) == p.len_out && srtp::red_src_cap(p, src_cap) >= p.len_out);
    if (p.len_out > dst_cap) { // a wrap that does not fit: nothing is moved
        CHECK(nj.copy_bytes == 0);
        return;
    }
    CHECK(nj.copy_bytes == up16(p.len_out) && nj.copy_bytes <= up16(dst_cap));
    // the two regions, exactly; the source's tail behind c is the region's, not the packet's
    Bytes src((size_t)up16(src_cap), 0xA5), dst((size_t)up16(dst_cap), 0xEE);
    memcpy(src.data(), pkt.data(), (size_t)c);
    const Bytes before(src);
    const int ws = j.copy_bytes / 16, wd = nj.copy_bytes / 16;
    CHECK(ws > 0 && 16 * ws <= (int)src.size());
    for (int q = 0; q < wd; q++) {
        const int sq = srtp::red_src_piece(q, ws), sw = srtp::red_src_word(q, p.shift, ws);
        CHECK(sq >= 0 && sq < ws && sw >= 0 && sw < 4 * ws);
        const uint8_t *a = src.data() + 16 * sq;
        const FanoutPiece A{le32(a), le32(a + 4), le32(a + 8), le32(a + 12)};
        const uint32_t nb = le32(src.data() + 4 * sw);
        const FanoutPiece o = srtp::red_piece(A, nb, q, p.shift, p.h, (uint32_t)p.ins, (uint32_t)p.pt);
        uint8_t *d = dst.data() + 16 * q;
        put_le32(d, o.w0);
        put_le32(d + 4, o.w1);
        put_le32(d + 8, o.w2);
        put_le32(d + 12, o.w3);
        // the piece against the byte-wise restatement, as far as the new packet goes
        for (int i = 16 * q; i < 16 * q + 16 && i < p.len_out; i++)
            if (d[i - 16 * q] != ref[(size_t)i]) {
                CHECK(d[i - 16 * q] == ref[(size_t)i]);
                break;
            }
        pieces++;
    }
    CHECK(src == before);
    for (size_t i = (size_t)nj.copy_bytes; i < dst.size(); i++) // nothing behind the new packet's pieces
        if (dst[i] != 0xEE) {
            CHECK(dst[i] == 0xEE);
            break;
        }
    for (int i = 0; i < p.len_out; i++) // what the later walk reads
        if (srtp::red_byte(rd, i, p) != ref[(size_t)i]) {
            CHECK(srtp::red_byte(rd, i, p) == ref[(size_t)i]);
            break;
        }
    // shift 0 is the identity
    const FanoutPiece A{1u, 2u, 3u, 4u};
    const FanoutPiece same = srtp::red_piece(A, 9u, 0, 0, 16, 7u, 5u);
    CHECK(same.w0 == 1u && same.w1 == 2u && same.w2 == 3u && same.w3 == 4u);
}

static Bytes packet(int c, int cc, bool x, int l0, int l1, int at_h) {
    Bytes b((size_t)c);
    for (int i = 0; i < c; i++) b[(size_t)i] = (uint8_t)(i * 7 + 3) & 0x7F;
    b[0] = (uint8_t)(0x80 | (x ? 0x10 : 0) | cc);
    b[1] = 0x80 | 96; // marker set, PT 96
    if (x) {
        const int p = 12 + 4 * cc + 2;
        if (p < c) b[(size_t)p] = (uint8_t)l0;
        if (p + 1 < c) b[(size_t)p + 1] = (uint8_t)l1;
    }
    int h;
    if (header_length(b, &h) && h >= 0 && h < c && at_h >= 0) b[(size_t)h] = (uint8_t)at_h;
    return b;
}

int main() {
    static const int lens[] = {0, 1, 2, 0x7F, 0x80, 0xFF};
    for (int c = 12; c <= 96; c++)
        for (int cc = 0; cc <= 2; cc++)
            for (int x = 0; x <= 1; x++)
                for (int l0 : lens)
                    for (int l1 : lens) {
                        if (!x && (l0 || l1)) continue;
                        for (int v = 0; v < 256; v++) {
                            const Bytes b = packet(c, cc, x != 0, l0, l1, v);
                            int h;
                            const bool in = header_length(b, &h) && h >= 0 && h < c;
                            if (!in && v) continue; // no byte at h to vary
                            for (int mode = srtp::kRedStrip; mode <= srtp::kRedWrap; mode++) {
                                one(b, mode, 96, c + 8, c + 8);
                                if (v == 0x45) {
                                    one(b, mode, 97, c + 8, c + 8);  // PT mismatch
                                    one(b, mode, 96, c, c);          // wrap does not fit
                                    one(b, mode, 96, c + 1, c + 1);  // fits exactly
                                    one(b, mode, 96, c + 8, c - 1);  // truncated: not asked
                                }
                            }
                        }
                    }
    // a header's end at 0, 4 and 8: an extension length of -(4 + CC) .. -(2 + CC) words
    for (int c = 12; c <= 40; c++)
        for (int cc = 0; cc <= 2; cc++)
            for (int k = 2; k <= 4; k++) {
                Bytes b = packet(c, cc, true, 0xFF, 256 - (k + cc), -1);
                for (int mode = srtp::kRedStrip; mode <= srtp::kRedWrap; mode++) one(b, mode, 96, c + 8, c + 8);
                b[(size_t)(4 * (4 - k))] &= 0x7F; // F clear at the header's end where it is not byte 0
                b[0] |= 0x80;
                for (int mode = srtp::kRedStrip; mode <= srtp::kRedWrap; mode++) one(b, mode, 96, c + 8, c + 8);
            }
    // version, the predicate's RTCP quirk, piece boundaries of a long copy
    for (int c : {1023, 1024, 1025, 2047, 2048, 2049})
        for (int pt : {96, 72, 83, 84}) {
            Bytes b = packet(c, 1, true, 0, 2, 0x45);
            b[1] = (uint8_t)(0x80 | pt);
            for (int mode = srtp::kRedStrip; mode <= srtp::kRedWrap; mode++) one(b, mode, pt, c + 8, c + 8);
            b[0] = (uint8_t)((b[0] & 0x3F) | 0x40);
            for (int mode = srtp::kRedStrip; mode <= srtp::kRedWrap; mode++) one(b, mode, pt, c + 8, c + 8);
        }
    // records that switch the step off
    {
        const FanoutJob j = srtp::fanout_job(0, 1, 64, 64, 0, 64, 0u);
        CHECK(srtp::red_wanted(j, 64, 64, 64, 1u, 96u, 0u) == 64);
        CHECK(srtp::red_wanted(j, 64, 64, 64, 0u, 96u, 0u) == 0 && srtp::red_wanted(j, 64, 64, 64, 3u, 96u, 0u) == 0);
        CHECK(srtp::red_wanted(j, 64, 64, 64, 1u, 128u, 0u) == 0 && srtp::red_wanted(j, 64, 64, 64, 2u, 96u, 1u) == 0);
        const FanoutJob s = srtp::fanout_job(0, 1, 64, 64, 0, 64, srtp::kFanFlagSkip);
        CHECK(srtp::red_wanted(s, 64, 64, 64, 1u, 96u, 0u) == 0);
        const FanoutJob t = srtp::fanout_job(0, 1, 11, 64, 0, 64, 0u);
        CHECK(srtp::red_wanted(t, 11, 64, 64, 1u, 96u, 0u) == 0);
    }
    printf("fanout_red_check: %ld cases, %ld stripped, %ld wrapped, %ld dropped, %ld untouched, %ld pieces, "
           "%d failures\n",
           cases, stripped, wrapped, dropped, untouched, pieces, failures);
    return failures || !stripped || !wrapped || !dropped || !untouched ? 1 : 0;
}
