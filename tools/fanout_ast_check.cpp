// fanout_ast_check.cpp -- stand-alone check of the abs-send-time stamp rule
// (libjitsi_amd/csrc/fanout_job.h: fanout_ast_find, fanout_ast_piece and
// fanout_ast_bytes, the text k_fanout_ast compiles), for a sanitizer build (no
// GPU, no Python).  It sweeps the shapes tests/test_fanout_ast.py runs on the
// device -- the element on every residue mod 16 of pieces 0/1, 1/2, 63/64 and
// 127/128, behind 0, 1 and 15 CSRCs, first, last and behind elements of every
// len; the reference's quirks (length bytes >= 0x80, length 0, the four
// overshoot bytes, padding, ID 0, a first match with len != 2, a packet or a
// destination that ends inside the element, a header that claims more than the
// packet holds, V != 2, X clear, another profile word); records that are off
// or carry ID 16 or 255; skipped entries -- and pseudo-random packets.  Every
// copy is replayed 16 bytes at a time through fanout_ast_piece between heap
// buffers of exactly the two regions' rounded sizes, the walk reading through
// a reader that refuses any index outside [0, c), and compared with a separate
// byte-wise restatement of AbsSendTimeEngine.transform / replaceAbsSendTime
// (AbsSendTimeEngine.java:46-152) over an int8_t buffer of exactly c bytes, as
// Java has it.  Nothing behind the copy may be written and the source must be
// unchanged; AddressSanitizer sees any byte outside either region.
//
//   make -C tools fanout_ast_check      (built with -fsanitize=address,undefined)
//   tools/fanout_ast_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/fanout_job.h"

using srtp::FanoutJob;
using srtp::FanoutPiece;

static int failures = 0;
static long cases = 0, replayed = 0, stamped = 0;
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

// ---- the reference, restated with Java's types: byte[] buf of exactly the packet, int arithmetic
static void java_set_timestamp(std::vector<int8_t> &buf, int off, int timestamp) {
    buf[(size_t)off] = (int8_t)(timestamp >> 16);
    buf[(size_t)off + 1] = (int8_t)(timestamp >> 8);
    buf[(size_t)off + 2] = (int8_t)timestamp;
}
static void java_replace(std::vector<int8_t> &buf, int extensionID, int timestamp) {
    const int length = (int)buf.size();
    int extensionOffset = 0;
    extensionOffset += 12;
    extensionOffset += (buf[0] & 0x0f) * 4;
    extensionOffset += 2;
    if (extensionOffset + 1 < length) {
        // buf[x] << 8 | buf[x + 1] on promoted, sign-extended bytes (times 256: the shift of a negative int)
        int lengthInWords = ((int)buf[(size_t)extensionOffset] * 256) | (int)buf[(size_t)extensionOffset + 1];
        int lengthInBytes = 4 * (1 + lengthInWords);
        extensionOffset += 2;
        int innerOffset = 0;
        while (extensionOffset < length && innerOffset < lengthInBytes) {
            int id = (buf[(size_t)extensionOffset] & 0xf0) >> 4;
            int len = buf[(size_t)extensionOffset] & 0x0f;
            if (id == extensionID) {
                if (len == 2 && extensionOffset + 3 < length) java_set_timestamp(buf, extensionOffset + 1, timestamp);
                return;
            } else {
                innerOffset += 1 + len + 1;
                extensionOffset += 1 + len + 1;
            }
        }
    }
}
static void java_transform(std::vector<int8_t> &buf, int extensionID, int timestamp) {
    if (extensionID != -1 && buf.size() >= 12 && ((buf[0] & 0xc0) >> 6) == 2 && (buf[0] & 0x10) == 0x10)
        java_replace(buf, extensionID, timestamp);
}

struct Record {
    uint32_t value;
    uint8_t id, on;
    uint16_t reserved;
};

struct Reader { // what the rule may read: bytes [0, c) of the source
    const uint8_t *p;
    int c;
    int operator()(int i) const {
        if (i < 0 || i >= c) {
            CHECK(i >= 0 && i < c);
            return 0;
        }
        return p[i];
    }
};

static uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void put_le32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// pkt: the source region's bytes (sc of them; the rest of the rounded region is a pattern)
static void one(const Bytes &pkt, int L, int sc, int dc, uint32_t fl, int st, const Record &r) {
    cases++;
    const FanoutJob j = srtp::fanout_job(0, 1, L, sc, st, dc, fl);
    const bool skipped = st != 0 || (fl & srtp::kFanFlagSkip);
    const int c = imin(L, imin(sc, dc));
    Bytes src((size_t)up16(sc)), dst((size_t)up16(dc));
    for (size_t i = 0; i < src.size(); i++) src[i] = i < pkt.size() ? pkt[i] : (uint8_t)(i * 7 + 3);
    const Bytes before(src);
    uint8_t *dp = dst.data();
    if (!dst.empty()) memset(dp, 0xEE, dst.size());
    const Reader rd{src.data(), c};
    const int at = srtp::fanout_ast_find(rd, j, L, sc, dc, r.on, r.id);
    CHECK(at == -1 || (at >= 13 && at + 2 < c && at + 2 < j.copy_bytes)); // every stamped byte is one the copy wrote
    if (skipped || !r.on || r.id > 15 || c < 12) CHECK(at == -1);
    // the copy as k_fanout_ast makes it: a piece is loaded, passed through the select, stored
    for (int o = 0; o < j.copy_bytes; o += 16) {
        const int q = o / 16;
        uint8_t piece[16];
        memcpy(piece, src.data() + o, 16);
        if (at >= 0 && q >= (at >> 4) && q <= ((at + 2) >> 4)) {
            const FanoutPiece p = srtp::fanout_ast_piece(
                FanoutPiece{le32(piece), le32(piece + 4), le32(piece + 8), le32(piece + 12)}, q, at, r.value);
            put_le32(piece, p.w0);
            put_le32(piece + 4, p.w1);
            put_le32(piece + 8, p.w2);
            put_le32(piece + 12, p.w3);
        } else if (at >= 0) { // outside the predicate the function changes nothing either
            const FanoutPiece p = srtp::fanout_ast_piece(
                FanoutPiece{le32(piece), le32(piece + 4), le32(piece + 8), le32(piece + 12)}, q, at, r.value);
            CHECK(p.w0 == le32(piece) && p.w1 == le32(piece + 4) && p.w2 == le32(piece + 8) && p.w3 == le32(piece + 12));
        }
        memcpy(dp + o, piece, 16);
    }
    CHECK(src == before);
    if (skipped) CHECK(j.copy_bytes == 0);
    if (!skipped && c > 0) {
        std::vector<int8_t> ref((size_t)c);
        memcpy(ref.data(), before.data(), (size_t)c);
        java_transform(ref, r.on && r.id <= 15 ? (int)r.id : -1, (int)(r.value & 0x00FFFFFFu));
        CHECK(memcmp(dp, ref.data(), (size_t)c) == 0);
        CHECK(memcmp(dp + c, before.data() + c, (size_t)(j.copy_bytes - c)) == 0); // the last piece's tail
        if (memcmp(ref.data(), before.data(), (size_t)c) != 0) stamped++;
        if (at >= 0) {
            const srtp::FanoutBytes b = srtp::fanout_ast_bytes(r.value);
            CHECK(dp[at] == b.b0 && dp[at + 1] == b.b1 && dp[at + 2] == b.b2);
        }
    }
    for (int i = j.copy_bytes; i < (int)dst.size(); i++) // nothing behind the copy
        if (dp[i] != 0xEE) {
            CHECK(dp[i] == 0xEE);
            break;
        }
    replayed++;
}

// ---- packets
static void element(Bytes &b, int id, int len_field, uint8_t fill) {
    b.push_back((uint8_t)(id << 4 | len_field));
    for (int i = 0; i <= len_field; i++) b.push_back((uint8_t)(fill + i));
}
// `front` bytes of other elements (0, or at least 2), the abs-send-time element (ID 3), a last element
static Bytes body_with(int front, bool last) {
    Bytes b;
    while (front > 0) {
        int take = front >= 19 ? 17 : front; // never leave a single byte
        if (front > 17 && front < 19) take = 16;
        element(b, 5, take - 2, 0x40);
        front -= take;
    }
    element(b, 3, 2, 0xA0);
    if (last) element(b, 7, 3, 0x70);
    while (b.size() % 4) b.push_back(0);
    while (((b.size() / 4) & 0xFF) >= 0x80) b.insert(b.end(), 4, 0); // a word count whose low byte is below 0x80
    return b;
}
static Bytes packet(int b0, const Bytes &body, int words, int profile, int payload) {
    Bytes p = {(uint8_t)b0, 96, 0x12, 0x34, 1, 2, 3, 4, 0xAA, 0xBB, 0xCC, 0xDD};
    for (int k = 0; k < (b0 & 15); k++)
        for (int i = 0; i < 4; i++) p.push_back((uint8_t)(0xC0 + k + i));
    p.push_back((uint8_t)(profile >> 8));
    p.push_back((uint8_t)profile);
    p.push_back((uint8_t)(words >> 8));
    p.push_back((uint8_t)words);
    p.insert(p.end(), body.begin(), body.end());
    for (int i = 0; i < payload; i++) p.push_back((uint8_t)(0x11 * (i % 15 + 1)));
    return p;
}

static const Record kRecords[] = {{0x00C1D2E3u, 3, 1, 0},  {0xFF010203u, 3, 1, 0xFFFF}, {0x00C1D2E3u, 3, 0, 0},
                                  {0x00C1D2E3u, 16, 1, 0}, {0x00C1D2E3u, 255, 1, 0},    {0x00C1D2E3u, 0, 1, 0},
                                  {0x00C1D2E3u, 5, 1, 0},  {0x00C1D2E3u, 7, 2, 0},      {0x00000000u, 3, 255, 0}};

// the packet whole, and cut by its length and by the destination around every place of interest
static void shapes(const Bytes &p, int around) {
    const int n = (int)p.size();
    for (const Record &r : kRecords) {
        one(p, n, n, n + 10, 0u, 0, r);
        for (int d = -4; d <= 6; d++) {
            const int cut = around + d;
            if (cut < 0 || cut > n) continue;
            one(p, cut, n, n + 10, 0u, 0, r);  // the packet ends there
            one(p, n, n, cut, 0u, 0, r);       // the destination does
            one(p, n, cut, n + 10, 0u, 0, r);  // the source region does
        }
    }
    one(p, n, n, n + 10, srtp::kFanFlagSkip, 0, kRecords[0]);
    one(p, n, n, n + 10, 0u, 2, kRecords[0]);
    for (int c = 0; c <= 13; c++) one(p, n, n, c, 0u, 0, kRecords[0]);
}

int main() {
    // placement: the first stamped byte on every residue of the piece pairs 0/1, 1/2, 63/64, 127/128
    for (int cc : {0, 1, 15})
        for (int base : {0, 16, 63 * 16, 127 * 16})
            for (int res = 0; res < 16; res++) {
                const int first = 12 + 4 * cc + 4 + 1; // the stamp's offset with the element first
                int front = base + res - first;
                while (front < 0 || front == 1) front += 16;
                const Bytes body = body_with(front, true);
                const Bytes p = packet(0x90 | cc, body, (int)body.size() / 4, 0xBEDE, 40);
                shapes(p, first + front);
            }
    // the element first, last, and behind an element of every len
    for (int cc : {0, 1, 15}) {
        for (int len = 0; len < 16; len++) {
            const Bytes body = body_with(len + 2, len & 1);
            shapes(packet(0x90 | cc, body, (int)body.size() / 4, 0xBEDE, 20), 12 + 4 * cc + 4 + len + 2 + 1);
        }
        const Bytes body = body_with(0, false);
        shapes(packet(0x90 | cc, body, (int)body.size() / 4, 0xBEDE, 0), 12 + 4 * cc + 4 + 1);
    }
    // the quirks
    {
        const Bytes body = body_with(6, true);
        const int w = (int)body.size() / 4, at = 16 + 6 + 1;
        for (int words : {w, 0, 1, 0x0080, 0x00FF, 0x8000, 0x8001, 0x7F7F, 0xFFFF, 0x7FFF, w + 1000})
            for (int profile : {0xBEDE, 0x1000, 0x0000, 0xFFFF})
                shapes(packet(0x90, body, words, profile, 30), at);
        for (int b0 : {0x80, 0x10, 0x50, 0xD0, 0x00, 0xB0, 0x9F}) shapes(packet(b0, body, w, 0xBEDE, 30), at);
        // a match in the four bytes past the declared extension, and one just behind them
        for (int past : {0, 1, 2, 3, 4, 5}) {
            Bytes b;
            element(b, 5, 5, 0x40); // 7 bytes
            b.push_back(0);         // one word boundary: 8 bytes = 2 words
            for (int i = 0; i < past; i++) b.push_back(0);
            element(b, 3, 2, 0xA0);
            while (b.size() % 4) b.push_back(0x11);
            shapes(packet(0x90, b, 2, 0xBEDE, 24), 16 + 8 + past + 1);
        }
        // padding in front of the element, odd and even counts; ID 0 against it (kRecords has one)
        for (int pad = 1; pad <= 6; pad++) {
            Bytes b((size_t)pad, 0);
            element(b, 3, 2, 0xA0);
            element(b, 7, 1, 0x70);
            while (b.size() % 4) b.push_back(0);
            shapes(packet(0x90, b, (int)b.size() / 4, 0xBEDE, 24), 16 + pad + 1);
        }
        // a first match whose len is not 2 in front of a good one
        for (int len : {0, 1, 3, 15}) {
            Bytes b;
            element(b, 3, len, 0x30);
            element(b, 3, 2, 0xA0);
            while (b.size() % 4) b.push_back(0);
            shapes(packet(0x90, b, (int)b.size() / 4, 0xBEDE, 24), 16 + len + 2 + 1);
        }
        // a header that claims more than the packet holds: CSRCs or an extension past the end
        for (int n = 12; n <= 24; n++) {
            Bytes p = packet(0x9F, Bytes(), 4, 0xBEDE, 0);
            p.resize((size_t)n);
            shapes(p, n);
        }
    }
    // pseudo-random packets: RTP-like first bytes, everything else noise, nibble-sized length words now and then
    uint32_t s = 12345u;
    auto rnd = [&s]() { return (s = s * 1664525u + 1013904223u) >> 8; };
    for (int k = 0; k < 60000; k++) {
        const int n = (int)(rnd() % 200u);
        Bytes p((size_t)n);
        for (int i = 0; i < n; i++) p[(size_t)i] = (uint8_t)rnd();
        const int cc = (int)(rnd() % 3u);
        if (n > 0 && k % 8) p[0] = (uint8_t)(0x90 | cc);
        const int lw = 12 + 4 * cc + 2;
        if (n > lw + 1 && k % 4) {
            p[(size_t)lw] = 0;
            p[(size_t)lw + 1] = (uint8_t)(rnd() % 24u);
        }
        const Record r = {rnd(), (uint8_t)(k % 5 ? rnd() % 16u : rnd() % 256u), (uint8_t)(k % 7 ? 1 : 0), (uint16_t)rnd()};
        one(p, n, n, k % 3 ? n + 16 : (int)(rnd() % 220u), 0u, 0, r);
    }
    printf("fanout_ast_check: %ld cases, %ld copies replayed, %ld stamped, %d failures\n", cases, replayed, stamped,
           failures);
    return failures || stamped == 0 ? 1 : 0;
}
