#!/usr/bin/env python3
"""Writes tests/golden/gcm_rfc7714.json: SRTP and SRTCP packets of the RFC 7714
AEAD profiles sealed by OpenSSL (EVP AES-GCM through ctypes), so that the
engine's output has an answer that passes through neither the engine's own
GF(2^128) arithmetic nor the Python GHASH of tests/gcm_ref.py.

Only the key derivation (AES in counter mode, RFC 7714 11) and the layout of
IV, AAD and trailer (RFC 7714 8, 9) come from tests/gcm_ref.py; the AEAD itself
is OpenSSL's.  Each stream is one master key / 12-byte master salt and a list
of packets in send order, with the ROC or SRTCP index each was sealed under.

    python tools/make_gcm_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gcm_ref as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gcm_rfc7714.json")


def srtp_stream(klen, seed, ssrc, shapes, seq0):
    key, salt = G.payload(klen, seed), G.payload(12, seed + 1)
    enc, ssalt = G.derive(key, salt, False)
    pkts = []
    for i, (plen, csrcs, ext) in enumerate(shapes):
        seq = (seq0 + i) & 0xFFFF
        roc = (seq0 + i) >> 16
        pkt = G.rtp_packet(ssrc, seq, G.payload(plen, seed + 10 + i), csrcs, ext)
        h = len(pkt) - plen
        ct, tag = G.openssl_gcm(enc, G.rtp_iv(ssalt, pkt[8:12], roc, seq), pkt[:h], pkt[h:])
        pkts.append({"in": pkt.hex(), "out": (pkt[:h] + ct + tag).hex(), "roc": roc})
    return {"kind": 0, "key": key.hex(), "salt": salt.hex(), "policy": list(G.policy(klen)), "packets": pkts}


def srtcp_stream(klen, seed, ssrc, lens):
    key, salt = G.payload(klen, seed), G.payload(12, seed + 1)
    enc, ssalt = G.derive(key, salt, True)
    pkts = []
    for index, blen in enumerate(lens):
        pkt = G.rtcp_packet(ssrc, G.payload(blen, seed + 10 + index))
        word = (0x80000000 | index).to_bytes(4, "big")
        ct, tag = G.openssl_gcm(enc, G.rtcp_iv(ssalt, pkt[4:8], index), pkt[:8] + word, pkt[8:])
        pkts.append({"in": pkt.hex(), "out": (pkt[:8] + ct + tag + word).hex(), "index": index})
    return {"kind": 1, "key": key.hex(), "salt": salt.hex(), "policy": list(G.policy(klen)), "packets": pkts}


def main():
    assert G.have_openssl(), "libcrypto not found"
    # (payload bytes, CSRCs, extension words or -1): block edges, AADs that are
    # no multiple of 16, a stream that crosses the sequence-number wrap
    shapes = [(0, 0, -1), (1, 0, -1), (15, 1, -1), (16, 0, 1), (17, 4, -1), (31, 0, 2), (32, 0, -1),
              (33, 2, 1), (48, 0, -1), (160, 0, -1), (1188, 0, -1)]
    streams = [srtp_stream(16, 100, 0x0A0B0C01, shapes, 65530),
               srtp_stream(32, 200, 0x0A0B0C02, shapes, 7),
               srtcp_stream(16, 300, 0x0A0B0C03, [4, 20, 21, 44, 100]),
               srtcp_stream(32, 400, 0x0A0B0C04, [8, 24, 36, 200])]
    with open(OUT, "w") as f:
        json.dump({"about": "RFC 7714 AEAD_AES_128/256_GCM packets sealed by OpenSSL (tools/make_gcm_golden.py)",
                   "streams": streams}, f, indent=0)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes,", sum(len(s["packets"]) for s in streams), "packets")


if __name__ == "__main__":
    main()
