// fec_recover_check.cpp -- stand-alone check of the FEC recovery rule
// (libjitsi_amd/csrc/fec_rx_job.h: fecrx_record_ok, fecrx_entry_ok, fecrx_head,
// fecrx_bit, fecrx_take, fecrx_plan, fecrx_status, fecrx_src_piece,
// fecrx_fec_word, fecrx_accumulate and fecrx_piece, the text k_fec_recover
// compiles), for a sanitizer build (no GPU, no Python).  The FEC packet and
// every candidate lie in heap buffers of exactly their length rounded up to 16
// -- what a region owns at the least -- with junk at and past the length.  The
// FEC header is read through a reader that aborts outside [0, len); then, for
// every output piece, the aligned 16-byte pieces and aligned 4-byte words the
// rule names are loaded, so that AddressSanitizer sees any load outside a
// buffer.  The packet is rebuilt piece by piece into a heap buffer of exactly
// fecrx_store_bytes and compared with a separate byte-wise restatement of
// FECReceiver.Reconstructor.setFecPacket and recover (transform/fec/
// FECReceiver.java:472-596): short and long masks, header lengths 12 / 16 / 20
// / 24, needed counts 0..47, member lengths around every piece boundary, the
// wrap quirk, duplicates, absent candidates, partial packets and every refusal.
//
//   make -C tools fec_recover_check      (built with -fsanitize=address,undefined)
//   tools/fec_recover_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "../libjitsi_amd/csrc/fec_rx_job.h"

using namespace srtp;

static int failures = 0;
static long records = 0, pieces = 0, refusals = 0, by_code[6] = {0, 0, 0, 0, 0, 0};
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static int up16(int v) { return (v + 15) & ~15; }
static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

struct Reader { // the packet's len bytes; anything else ends the program
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

// ---- the reference, restated over Java byte arrays.  code as SRTP_FECRX_*.
static int java_header_length(const Bytes &b, bool &oob) { // RawPacket.getHeaderLength
    int h = 12 + 4 * (b[0] & 0x0f);
    oob = false;
    if (b[0] & 0x10) {
        const int x = h + 2;
        if (x + 1 >= (int)b.size()) {
            oob = true;
            return 0;
        }
        h += 4 + (((int)(int8_t)b[(size_t)x] * 256) | b[(size_t)x + 1]) * 4; // Java's << 8 of a signed byte
    }
    return h;
}

static int reference(const Bytes &fec, const std::vector<Bytes> &present, uint32_t ssrc, Bytes &out) {
    out.clear();
    if (fec.size() < 12 || fec.size() > 65535) return kFecRxRefused;
    std::map<int, const Bytes *> media; // mediaPackets: put replaces
    for (const Bytes &p : present) media[(p[2] << 8) | p[3]] = &p;
    bool oob;
    const int hl = java_header_length(fec, oob);
    if (oob || hl < 0 || hl + 14 > (int)fec.size()) return kFecRxRefused; // the defined deviation
    int idx = hl;
    const int mask_len = (fec[(size_t)idx] & 0x40) == 0 ? 2 : 6;
    if (mask_len == 6 && hl + 18 > (int)fec.size()) return kFecRxRefused;
    const int base = (fec[(size_t)hl + 2] << 8) | fec[(size_t)hl + 3];
    idx += 12;
    std::vector<const Bytes *> needed;
    int num_missing = 0, sequence_number = -1;
    for (int i = 0; i < mask_len && num_missing <= 1; i++)
        for (int j = 0; j < 8; j++) {
            if ((fec[(size_t)(idx + i)] & (1 << (7 - j) & 0xff)) != 0) {
                auto it = media.find(base + i * 8 + j);
                if (it != media.end())
                    needed.push_back(it->second);
                else {
                    sequence_number = base + i * 8 + j;
                    num_missing++;
                }
            }
            if (num_missing > 1) break;
        }
    if (num_missing == 0) return kFecRxComplete;
    if (num_missing != 1) return kFecRxWait;
    idx = hl; // recover
    int length_recovery = (fec[(size_t)idx + 8] & 0xff) << 8 | (fec[(size_t)idx + 9] & 0xff);
    for (const Bytes *p : needed) length_recovery ^= (int)p->size() - 12;
    length_recovery &= 0xffff;
    Bytes rec((size_t)length_recovery + 12, 0);
    for (int i = 0; i < 8; i++) rec[(size_t)i] = fec[(size_t)(idx + i)];
    for (const Bytes *p : needed)
        for (int i = 0; i < 8; i++) rec[(size_t)i] ^= (*p)[(size_t)i];
    rec[0] &= 0x3f;
    rec[0] |= 0x80;
    const bool long_mask = (fec[(size_t)idx] & 0x40) != 0;
    idx += 10;
    const int protection_length = ((fec[(size_t)idx] & 0xff) << 8) | (fec[(size_t)idx + 1] & 0xff);
    if (protection_length < length_recovery) return kFecRxPartial;
    idx += 4;
    if (long_mask) idx += 4;
    if (idx + length_recovery > (int)fec.size()) return kFecRxRefused; // the defined deviation
    for (int i = 0; i < length_recovery; i++) rec[12 + (size_t)i] = fec[(size_t)(idx + i)];
    for (const Bytes *p : needed)
        for (int i = 12; i < length_recovery + 12 && i < (int)p->size(); i++) rec[(size_t)i] ^= (*p)[(size_t)i];
    rec[8] = (uint8_t)(ssrc >> 24);
    rec[9] = (uint8_t)(ssrc >> 16);
    rec[10] = (uint8_t)(ssrc >> 8);
    rec[11] = (uint8_t)ssrc;
    rec[2] = (uint8_t)(sequence_number >> 8);
    rec[3] = (uint8_t)sequence_number;
    out = rec;
    return kFecRxRecovered;
}

// ---- a sender for the fixtures: RFC 5109 over `media` at mask positions pos[], an RTP header of hl bytes
static Bytes make_fec(const std::vector<Bytes> &media, const std::vector<int> &pos, int base, int hl, bool lng) {
    int plen = 0;
    for (const Bytes &m : media) plen = (int)m.size() - 12 > plen ? (int)m.size() - 12 : plen;
    const int pay = hl + (lng ? 18 : 14);
    Bytes f((size_t)pay + (size_t)plen, 0);
    for (int i = 0; i < hl; i++) f[(size_t)i] = (uint8_t)rnd();
    if (hl == 12)
        f[0] = 0x80;
    else if (hl == 16 && (rnd() & 1))
        f[0] = 0x81; // one CSRC
    else {           // an extension of (hl - 16) / 4 words
        f[0] = 0x90;
        f[14] = 0;
        f[15] = (uint8_t)((hl - 16) / 4);
    }
    int lx = 0;
    for (size_t k = 0; k < media.size(); k++) {
        const Bytes &m = media[k];
        for (int i = 0; i < 8; i++) f[(size_t)(hl + i)] ^= m[(size_t)i];
        lx ^= (int)m.size() - 12;
        for (size_t i = 12; i < m.size(); i++) f[(size_t)pay + i - 12] ^= m[i];
        f[(size_t)(hl + 12 + pos[k] / 8)] |= (uint8_t)(0x80 >> (pos[k] % 8));
    }
    f[(size_t)hl] = (uint8_t)((f[(size_t)hl] & ~0x40) | (lng ? 0x40 : 0));
    f[(size_t)hl + 2] = (uint8_t)(base >> 8);
    f[(size_t)hl + 3] = (uint8_t)base;
    f[(size_t)hl + 8] = (uint8_t)(lx >> 8);
    f[(size_t)hl + 9] = (uint8_t)lx;
    f[(size_t)hl + 10] = (uint8_t)(plen >> 8);
    f[(size_t)hl + 11] = (uint8_t)plen;
    return f;
}

static Bytes packet(int seq, int len) {
    Bytes b((size_t)len);
    for (int i = 0; i < len; i++) b[(size_t)i] = (uint8_t)rnd();
    b[0] = (uint8_t)(0x80 | (b[0] & 0x3F));
    b[2] = (uint8_t)(seq >> 8);
    b[3] = (uint8_t)seq;
    return b;
}

// ---- the rule, driven the way the kernel drives it
struct Region {
    uint8_t *p; // exactly up16(len) bytes on the heap, junk behind len
    int len;
};
static Region region_of(const Bytes &b) {
    Region r{(uint8_t *)malloc((size_t)up16((int)b.size()) + (b.empty() ? 16 : 0)), (int)b.size()};
    for (int i = 0; i < up16(r.len); i++) r.p[i] = i < r.len ? b[(size_t)i] : (uint8_t)rnd();
    return r;
}
static uint32_t load32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// candidates: the list as the record names it; an empty Bytes is an absent candidate (status not OK, short len).
static int one(const Bytes &fecb, const std::vector<Bytes> &cands, uint32_t ssrc, int out_cap) {
    std::vector<Bytes> present;
    for (const Bytes &c : cands)
        if (c.size() >= 12) present.push_back(c);
    Bytes want;
    const int want_code = reference(fecb, present, ssrc, want);
    records++;
    by_code[want_code < 0 ? 5 : want_code]++;
    CHECK(fecrx_record_ok(0, (uint32_t)cands.size(), (uint32_t)cands.size()));
    const Region F = region_of(fecb);
    FecRxPlan p{kFecRxRefused, 0, 0, 0};
    FecRxHead h{};
    h.code = kFecRxRefused;
    std::vector<Region> mem;
    std::vector<int> needed;
    if (fecrx_entry_ok(0, F.len, F.len)) h = fecrx_head(Reader{F.p, F.len}, F.len);
    if (h.code == 0) {
        CHECK(h.hl >= 0 && h.hl % 4 == 0 && h.hl + 14 + h.lm <= F.len);
        for (const Bytes &c : cands) mem.push_back(region_of(c));
        uint64_t covered = 0;
        int len_xor = 0;
        for (int k = (int)cands.size() - 1; k >= 0; k--) {
            const Region &m = mem[(size_t)k];
            if (!fecrx_entry_ok(0, m.len, m.len)) continue; // absent: nothing of it is read
            if (fecrx_take(covered, fecrx_bit(fecrx_key(load32(m.p)), h))) {
                needed.push_back(k);
                len_xor ^= m.len - 12;
            }
        }
        p = fecrx_plan(h, covered, len_xor, F.len);
    }
    CHECK(p.code == want_code);
    CHECK(p.len_out == (int)want.size());
    const int status = fecrx_status(p, out_cap);
    CHECK(status == (want_code != kFecRxRecovered ? 9 : (int)want.size() <= out_cap ? 0 : 7));
    if (p.code == kFecRxRecovered && p.code == want_code) {
        const int store = fecrx_store_bytes(p.len_out, out_cap);
        CHECK(store == up16(p.len_out < out_cap ? p.len_out : out_cap) && store <= up16(out_cap));
        uint8_t *out = (uint8_t *)malloc(store ? (size_t)store : 1);
        for (int q = 0; q < store / 16; q++) {
            uint32_t W[5];
            for (int i = 0; i < 5; i++) {
                const uint8_t *w = F.p + 4 * fecrx_fec_word(q, i, h, F.len); // ASan: inside up16(len)
                CHECK(w + 4 <= F.p + up16(F.len));
                W[i] = load32(w);
            }
            FecRxWindow a{0, 0, 0, 0};
            for (int k : needed) {
                const Region &m = mem[(size_t)k];
                const uint8_t *P = m.p + 16 * fecrx_src_piece(q, m.len);
                CHECK(P + 16 <= m.p + up16(m.len));
                fecrx_accumulate(a, FanoutPiece{load32(P), load32(P + 4), load32(P + 8), load32(P + 12)}, q, m.len);
            }
            if (!needed.empty()) { // an empty batch slot: the last member's piece 0 with len 0
                const uint8_t *P = mem[(size_t)needed.back()].p;
                FecRxWindow b = a;
                fecrx_accumulate(b, FanoutPiece{load32(P), load32(P + 4), load32(P + 8), load32(P + 12)}, q, 0);
                CHECK(memcmp(&a, &b, sizeof a) == 0);
            }
            const FanoutPiece o = fecrx_piece(a, W[0], W[1], W[2], W[3], W[4], q, h, p, F.len, ssrc);
            memcpy(out + 16 * q, &o, 16);
            pieces++;
        }
        for (int i = 0; i < store && i < p.len_out; i++)
            if (out[i] != want[(size_t)i]) {
                CHECK(out[i] == want[(size_t)i]);
                if (failures < 20)
                    printf("  hl %d long %d len_out %d needed %zu byte %d: %02x, want %02x\n", h.hl, h.lm, p.len_out,
                           needed.size(), i, out[i], want[(size_t)i]);
                break;
            }
        free(out);
    }
    for (Region &m : mem) free(m.p);
    free(F.p);
    return p.code;
}

// A group of `count` packets at mask positions pos[] (ascending), of which `lost` (indices) are withheld.
static int group(const std::vector<int> &lens, const std::vector<int> &pos, int base, int hl, bool lng,
                 const std::vector<int> &lost, int extra_cands, int cap_delta, int lost_len = -1) {
    std::vector<Bytes> media;
    for (size_t k = 0; k < lens.size(); k++) media.push_back(packet((base + pos[k]) & 0xFFFF, lens[k]));
    const Bytes fec = make_fec(media, pos, base, hl, lng);
    std::vector<Bytes> cands;
    for (int i = 0; i < extra_cands; i++) // outside the mask: in front of the base, or another stream's numbers
        cands.push_back(packet((base - 1 - (int)(rnd() % 200)) & 0xFFFF, 12 + (int)(rnd() % 60)));
    for (size_t k = 0; k < media.size(); k++) {
        bool gone = false;
        for (int l : lost) gone = gone || l == (int)k;
        if (!gone) cands.push_back(media[k]);
    }
    for (size_t i = cands.size(); i > 1; i--) std::swap(cands[i - 1], cands[rnd() % i]); // any order
    int want_len = lost.size() == 1 ? lens[(size_t)lost[0]] : 0;
    if (lost_len >= 0) want_len = lost_len;
    return one(fec, cands, rnd(), want_len + cap_delta);
}

static void refusals_sweep() {
    CHECK(fecrx_record_ok(0, 0, 0) && fecrx_record_ok(0, 64, 64) && fecrx_record_ok(7, 64, 71));
    CHECK(!fecrx_record_ok(0, 65, 100) && !fecrx_record_ok(0, 255, 1000) && !fecrx_record_ok(8, 64, 71) &&
          !fecrx_record_ok(5, 0, 4) && !fecrx_record_ok(0xFFFFFFFFu, 2, 0xFFFFFFFFu));
    CHECK(fecrx_index_ok(0, 1) && fecrx_index_ok(6, 7) && !fecrx_index_ok(-1, 7) && !fecrx_index_ok(7, 7));
    CHECK(fecrx_entry_ok(0, 12, 12) && fecrx_entry_ok(0, 65535, 65535) && fecrx_entry_ok(0, 40, 41));
    CHECK(!fecrx_entry_ok(2, 40, 40) && !fecrx_entry_ok(9, 40, 40) && !fecrx_entry_ok(0, 11, 40) &&
          !fecrx_entry_ok(0, 0, 40) && !fecrx_entry_ok(0, -1, 40) && !fecrx_entry_ok(0, 41, 40) &&
          !fecrx_entry_ok(0, 40, -1) && !fecrx_entry_ok(0, 65536, 65536));
    refusals += 22;
    // the FEC packet cut short at every length: refused below hl + 14 (+ 4) and below the payload's end
    for (int hl : {12, 16, 20, 24})
        for (int lng = 0; lng < 2; lng++) {
            std::vector<Bytes> media{packet(100, 40), packet(101, 33), packet(102, 52)};
            const Bytes full = make_fec(media, {0, 1, 2}, 100, hl, lng != 0);
            for (int cut = 0; cut <= (int)full.size(); cut++) {
                const Bytes f(full.begin(), full.begin() + cut);
                const int code = one(f, {media[0], media[2]}, 5, 80);
                const int pay = hl + (lng ? 18 : 14);
                CHECK(code == (cut < pay + 33 - 12 ? kFecRxRefused : kFecRxRecovered));
                refusals++;
            }
        }
    { // an extension length that points past the packet, a negative one, and one whose two bytes are cut off
        std::vector<Bytes> media{packet(7, 30)};
        Bytes f = make_fec(media, {0}, 7, 16, false);
        f[0] = 0x90;
        f[14] = 0x7F;
        CHECK(one(f, {}, 1, 64) == kFecRxRefused);
        f[14] = 0x80; // (sbyte) -128 << 8: a header length far below 0
        CHECK(one(f, {}, 1, 64) == kFecRxRefused);
        f[14] = 0xFF;
        f[15] = 0xFC; // -4 words: hl = 0, the FEC header lies over the RTP header; the reference goes on
        Bytes w;
        CHECK(one(f, {}, 1, 64) == reference(f, {}, 1, w));
        Bytes g(f.begin(), f.begin() + 15);
        g[0] = 0x90;
        CHECK(one(g, {}, 1, 64) == kFecRxRefused);
        Bytes s(11, 0x80);
        CHECK(one(s, {}, 1, 64) == kFecRxRefused);
        refusals += 5;
    }
}

int main() {
    refusals_sweep();
    const int single[] = {12, 13, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1200, 2036};
    for (int hl : {12, 16, 20, 24})
        for (int lng = 0; lng < 2; lng++) {
            for (int len : single)
                for (int needed : {0, 1, 3, 4, 5, 15, 16, 47}) {
                    const int count = needed + 1;
                    if (count > (lng ? 48 : 16)) continue;
                    std::vector<int> pos;
                    for (int k = 0; k < count; k++) pos.push_back(k);
                    for (int delta : {20, 0, -1}) // an output region roomy, exact, one byte short
                        CHECK(group(std::vector<int>((size_t)count, len), pos, 3000 + (int)(rnd() % 1000), hl, lng != 0,
                                    {(int)(rnd() % (uint32_t)count)}, (int)(rnd() % (uint32_t)(65 - count)), delta) ==
                              kFecRxRecovered);
                }
            for (int rep = 0; rep < 60; rep++) { // mixed lengths, sparse masks, the lost one longer or shorter than the rest
                const int bits = lng ? 48 : 16, count = 1 + (int)(rnd() % (uint32_t)bits);
                std::vector<int> pos, lens;
                for (int k = 0; k < bits && (int)pos.size() < count; k++)
                    if ((int)(rnd() % (uint32_t)(bits - k)) < count - (int)pos.size()) pos.push_back(k);
                const int longest = single[rnd() % 14];
                for (size_t k = 0; k < pos.size(); k++) lens.push_back(12 + (int)(rnd() % (uint32_t)(longest - 11)));
                const int lost = (int)(rnd() % (uint32_t)pos.size());
                if (rep % 3 == 0) lens[(size_t)lost] = longest;
                if (rep % 3 == 1) lens[(size_t)lost] = 12;
                CHECK(group(lens, pos, (int)(rnd() % 60000), hl, lng != 0, {lost}, (int)(rnd() % (uint32_t)(65 - (int)pos.size())),
                            (int)(rnd() % 3) - 1) == kFecRxRecovered);
                CHECK(group(lens, pos, 500, hl, lng != 0, {}, 3, 0) == kFecRxComplete);
                if (pos.size() >= 2)
                    CHECK(group(lens, pos, 500, hl, lng != 0, {0, (int)pos.size() - 1}, 3, 0) == kFecRxWait);
            }
        }
    { // duplicates: the later of two candidates with one sequence number stands, whether or not it is the true one
        std::vector<Bytes> media{packet(10, 40), packet(11, 50), packet(12, 60)};
        const Bytes fec = make_fec(media, {0, 1, 2}, 10, 12, false);
        Bytes other = packet(11, 50); // another packet under the same number
        CHECK(one(fec, {media[0], other, media[1]}, 9, 100) == kFecRxRecovered);
        CHECK(one(fec, {media[0], media[1], other}, 9, 100) == kFecRxRecovered); // a wrong packet, as the reference
        CHECK(one(fec, {media[0], media[1], other, media[2], media[2]}, 9, 100) == kFecRxComplete);
        // absent candidates: shorter than 12, or none at all
        CHECK(one(fec, {media[0], Bytes(), media[1], Bytes(5, 1)}, 9, 100) == kFecRxRecovered);
        CHECK(one(fec, {Bytes(), Bytes()}, 9, 100) == kFecRxWait);
        CHECK(one(fec, {}, 9, 100) == kFecRxWait);
    }
    { // the wrap quirk: keys above 65535 are never found
        std::vector<Bytes> media;
        for (int k = 0; k < 4; k++) media.push_back(packet((65533 + k) & 0xFFFF, 40 + k));
        const Bytes fec = make_fec(media, {0, 1, 2, 3}, 65533, 12, false); // keys 65533, 65534, 65535, 65536
        CHECK(one(fec, media, 9, 100) == kFecRxRecovered); // complete, and yet "recovers" packet 0 again
        CHECK(one(fec, {media[0], media[1], media[3]}, 9, 100) == kFecRxWait); // one truly lost: two missing
        const Bytes fec2 = make_fec(media, {0, 1, 2, 3}, 65534, 12, false); // two keys past the wrap: waits for ever
        CHECK(one(fec2, media, 9, 100) == kFecRxWait);
    }
    { // partial: a protection length below the recovered length
        std::vector<Bytes> media{packet(20, 40), packet(21, 80)};
        Bytes fec = make_fec(media, {0, 1}, 20, 12, false);
        fec[12 + 11] = 27; // below 80 - 12
        CHECK(one(fec, {media[0]}, 9, 100) == kFecRxPartial);
        CHECK(one(fec, {media[1]}, 9, 100) == kFecRxPartial); // 28 wanted, 27 protected
        fec[12 + 11] = 28;
        CHECK(one(fec, {media[1]}, 9, 100) == kFecRxRecovered);
    }
    { // the largest entries
        std::vector<Bytes> media{packet(1, 65535 - 26), packet(2, 12)};
        const Bytes fec = make_fec(media, {0, 1}, 1, 12, false);
        CHECK(one(fec, {media[1]}, 9, 65535) == kFecRxRecovered);
        CHECK(one(fec, {media[0]}, 9, 12) == kFecRxRecovered);
    }
    printf("fec_recover_check: %ld records (%ld recovered, %ld complete, %ld waiting, %ld partial, %ld refused), "
           "%ld pieces, %ld refusal checks, %d failures\n",
           records, by_code[1], by_code[2], by_code[3], by_code[4], by_code[5], pieces, refusals, failures);
    return failures ? 1 : 0;
}
