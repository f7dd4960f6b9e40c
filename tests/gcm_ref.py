"""Test-side reference for the RFC 7714 AES-GCM profiles.

TEST INFRASTRUCTURE ONLY.  The C oracle has no AES-GCM, so the reference for
SRTP_AESGCM_ENCRYPTION lives here: a pure-Python restatement of RFC 7714 laid
over the orchestration order of the reference contexts (replay check,
authenticate, decrypt, update -- SRTPCryptoContext.java:572-642,
SRTCPCryptoContext.java:333-451) as oracle/pyref.py:354-457 restates them.  It
shares pyref's state machine (guess, replay_ok, update, header_len), its
Transformer / Factory objects and its AES building blocks, and adds GHASH on
Python integers (NIST SP 800-38D 6.3-6.4, bit by bit: nothing in common with
the engine's 4-bit tables), the RFC 7714 IVs and key derivation, and a
``process`` with pyref.process's contract.  T = 16 throughout.  The engine's
host AES-GCM and key derivation are pinned to it (tests/test_gcm_host.py); it is
also the reference a GPU path for these profiles has to match.

SRTP (RFC 7714 8.1, 7.1)
  IV = (0x0000 || SSRC || ROC || SEQ) ^ salt; AAD = the RTP header
  (getHeaderLength() bytes); plaintext = the rest.
  protect:   L + 16 > cap -> ERR_CAPACITY (before any state change); guess /
             replay as pyref; a header length that throws or is negative, or
             longer than L -> ERR_MALFORMED; else ciphertext || tag, L += 16,
             update.
  unprotect: replay check first; header length throws or is negative ->
             ERR_MALFORMED (length unchanged); L - 16 < header -> DROP_AUTH;
             tag mismatch -> DROP_AUTH (length max(0, L - 16), bytes
             untouched); else decipher in place (not with DISCARD / SILENCE),
             L -= 16, update.
SRTCP (RFC 7714 9.1-9.3)
  header(8) || ciphertext || tag(16) || E|index(4); IV = (0x0000 || SSRC ||
  0x0000 || 0|index) ^ salt; AAD = the first 8 bytes || the E|index word.
  protect:   L + 20 > cap -> ERR_CAPACITY; always E = 1, index = sentIndex,
             then sentIndex = (sentIndex + 1) & 0x7FFFFFFF.
  unprotect: L - 20 < 0 -> ERR_MALFORMED; 20 <= L < 28 -> DROP_AUTH (L - 20);
             E|index at L - 4, replay check as pyref; E = 1: open; E = 0
             (9.3): AAD = the packet up to the tag || the E|index word, no
             plaintext; tag mismatch -> DROP_AUTH (L - 20, bytes untouched);
             accepted: L -= 20, window and index as pyref.py:451-456.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util

import numpy as np

from oracle import pyref
from oracle.pyref import M32, M64, Throw, i32, i64, ishl1, lshl

GCM = 5  # SRTP_AESGCM_ENCRYPTION
T = 16
PROFILE_128, PROFILE_256 = 0x0007, 0x0008


def policy(klen: int):
    """(enc, enc_len, auth, auth_len, tag, salt_len) of AEAD_AES_{128,256}_GCM."""
    return (GCM, klen, 0, 0, T, 12)


# ------------------------------------------------------------ AES, both sizes
def expand_key(key: bytes):
    """FIPS-197 key expansion for 16- or 32-byte keys (pyref's is AES-128 only)."""
    if len(key) == 16:
        return pyref.expand_key(key)
    nk, nr = len(key) // 4, len(key) // 4 + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [pyref.SBOX[t[1]] ^ rcon, pyref.SBOX[t[2]], pyref.SBOX[t[3]], pyref.SBOX[t[0]]]
            rcon = pyref._xt(rcon)
        elif nk > 6 and i % nk == 4:
            t = [pyref.SBOX[b] for b in t]
        w.append([w[i - nk][k] ^ t[k] for k in range(4)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(nr + 1)]


def aes_block(rks, block: bytes) -> bytes:
    if len(rks) == 11:
        return pyref.aes_block(rks, block)
    nr = len(rks) - 1
    s = [b ^ k for b, k in zip(block, rks[0])]
    for r in range(1, nr + 1):
        s = [pyref.SBOX[s[4 * ((c + row) % 4) + row]] for c in range(4) for row in range(4)]
        if r < nr:
            x, t = pyref._xt, []
            for c in range(4):
                a0, a1, a2, a3 = s[4 * c:4 * c + 4]
                t += [x(a0) ^ x(a1) ^ a1 ^ a2 ^ a3, a0 ^ x(a1) ^ x(a2) ^ a2 ^ a3,
                      a0 ^ a1 ^ x(a2) ^ x(a3) ^ a3, x(a0) ^ a0 ^ a1 ^ a2 ^ x(a3)]
            s = t
        s = [b ^ k for b, k in zip(s, rks[r])]
    return bytes(s)


# ------------------------------------------------------------------- AES-GCM
_R = 0xE1 << 120


def gf_mult(x: int, y: int) -> int:
    """SP 800-38D 6.3, Algorithm 1: blocks as integers, bit 0 = the MSB."""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def ghash(h: int, aad: bytes, ct: bytes) -> int:
    y = 0
    for part in (aad, ct):
        for o in range(0, len(part), 16):
            y = gf_mult(y ^ int.from_bytes(part[o:o + 16].ljust(16, b"\0"), "big"), h)
    return gf_mult(y ^ ((len(aad) * 8) << 64) ^ (len(ct) * 8), h)


def _ctr(rks, iv: bytes, data: bytes) -> bytes:
    out = bytearray()
    for o in range(0, len(data), 16):
        ks = aes_block(rks, iv + (o // 16 + 2).to_bytes(4, "big"))
        out += bytes(a ^ b for a, b in zip(data[o:o + 16], ks))
    return bytes(out)


def _tag(rks, iv, aad, ct) -> bytes:
    h = int.from_bytes(aes_block(rks, bytes(16)), "big")
    s = ghash(h, aad, ct) ^ int.from_bytes(aes_block(rks, iv + b"\0\0\0\1"), "big")
    return s.to_bytes(16, "big")


def seal(rks, iv: bytes, aad: bytes, pt: bytes):
    ct = _ctr(rks, iv, pt)
    return ct, _tag(rks, iv, aad, ct)


def open_(rks, iv: bytes, aad: bytes, ct: bytes, tag: bytes):
    """The plaintext, or None on a tag mismatch."""
    if _tag(rks, iv, aad, ct) != bytes(tag):
        return None
    return _ctr(rks, iv, ct)


# ------------------------------------------------------- RFC 7714 11: the KDF
def derive(mk: bytes, ms: bytes, rtcp: bool):
    """Session key (len(mk) bytes) and 12-byte session salt: the AES-CM PRF of
    the key's size (RFC 3711 4.3 / RFC 6188) over the 12-byte master salt
    padded with two zero bytes; labels 0 / 3 and 2 / 5; no auth key."""
    rks = expand_key(mk)
    out = []
    for lab, n in zip((3, 5) if rtcp else (0, 2), (len(mk), 12)):
        iv = bytearray(ms[:12]) + b"\0\0"
        iv[7] ^= lab
        ks = b"".join(aes_block(rks, bytes(iv) + i.to_bytes(2, "big")) for i in range((n + 15) // 16))
        out.append(ks[:n])
    return out[0], out[1]


def rtp_iv(salt, ssrc: bytes, roc: int, seq: int) -> bytes:
    raw = b"\0\0" + bytes(ssrc) + (roc & M32).to_bytes(4, "big") + seq.to_bytes(2, "big")
    return bytes(a ^ b for a, b in zip(raw, salt))


def rtcp_iv(salt, ssrc: bytes, index: int) -> bytes:
    raw = b"\0\0" + bytes(ssrc) + b"\0\0" + (index & 0x7FFFFFFF).to_bytes(4, "big")
    return bytes(a ^ b for a, b in zip(raw, salt))


# ------------------------------------------------------------------ contexts
class GcmCtx:
    def __init__(self, pol, mk, ms, rtcp):
        self.policy = pol
        enc, self.salt = derive(bytes(mk)[:pol[1]], bytes(ms)[:12], rtcp)
        self.rks = expand_key(enc)
        self.roc = self.s_l = self.guessed = 0
        self.seq_set = False
        self.sent = self.recv = 0
        self.window = 0


class Transformer(pyref.Transformer):
    """pyref's transformer; contexts of a GCM policy are GcmCtx."""

    def get(self, ssrc, f):
        c = self.ctx.get(ssrc)
        if c is None and f is not None and not f.closed:
            rtcp = self.kind == 1
            pol = f.srtcp if rtcp else f.srtp
            c = GcmCtx(pol, f.mk, f.ms, rtcp) if pol[0] == GCM else pyref.Ctx(pol, f.mk, f.ms, rtcp)
            self.ctx[ssrc] = c
        return c

    def state(self, ssrc):
        """The context's state under the engine's srtp_ctx_state names."""
        c = self.ctx.get(ssrc)
        if c is None:
            return None
        return {"roc": c.roc, "s_l": c.s_l, "seq_num_set": int(c.seq_set), "guessed_roc": c.guessed,
                "replay_window": c.window & M64, "sent_index": c.sent, "received_index": c.recv}


Factory = pyref.Factory


def _header_len(buf, cap):
    h = pyref.header_len(buf, cap)
    if h < 0:  # a negative extension length: no such AAD
        raise Throw("negative header length")
    return h


def process_one(t, reverse, buf: bytearray, L, cap, flags):
    """(status, new length); non-GCM contexts go to pyref.process_one."""
    if L < 12 or L > cap:
        return 7, L
    rtp = t.kind == 0
    if rtp and reverse and (buf[0] & 0xC0) != 0x80:
        return 3, L
    ssrc = bytes(buf[8:12]) if rtp else bytes(buf[4:8])
    c = t.get(int.from_bytes(ssrc, "big"), t.rev if reverse else t.fwd)
    if c is None:
        return 4, L
    if c.policy[0] != GCM:
        return pyref.process_one(t, reverse, buf, L, cap, flags)
    if rtp:
        seq = (buf[2] << 8) | buf[3]
        if not reverse:
            if L + T > cap:
                return 5, L
            if not c.seq_set:
                c.seq_set, c.s_l = True, seq
            gi = pyref.guess(c, seq)
            if not pyref.replay_ok(c, gi):
                return 1, L
            try:
                h = _header_len(buf, cap)
            except Throw:
                return 6, L
            if h > L:
                return 6, L
            ct, tag = seal(c.rks, rtp_iv(c.salt, ssrc, c.guessed, seq), bytes(buf[:h]), bytes(buf[h:L]))
            buf[h:L] = ct
            buf[L:L + T] = tag
            pyref.update(c, seq, gi)
            return 0, L + T
        if not c.seq_set:
            c.seq_set, c.s_l = True, seq
        gi = pyref.guess(c, seq)
        if not pyref.replay_ok(c, gi):
            return 1, L
        try:
            h = _header_len(buf, cap)
        except Throw:
            return 6, L
        if L - T < h:
            return 2, max(0, L - T)
        L -= T
        pt = open_(c.rks, rtp_iv(c.salt, ssrc, c.guessed, seq), bytes(buf[:h]), bytes(buf[h:L]),
                   bytes(buf[L:L + T]))
        if pt is None:
            return 2, L
        if not (flags & 0x6):
            buf[h:L] = pt
        pyref.update(c, seq, gi)
        return 0, L
    # SRTCP
    if not reverse:
        if L + T + 4 > cap:
            return 5, L
        word = (c.sent | 0x80000000) & M32
        wb = word.to_bytes(4, "big")
        ct, tag = seal(c.rks, rtcp_iv(c.salt, ssrc, c.sent), bytes(buf[:8]) + wb, bytes(buf[8:L]))
        buf[8:L] = ct
        buf[L:L + T] = tag
        buf[L + T:L + T + 4] = wb
        c.sent = (c.sent + 1) & 0x7FFFFFFF
        return 0, L + T + 4
    if L - 4 - T < 0:
        return 6, L
    if L < 8 + T + 4:
        return 2, L - T - 4
    wb = bytes(buf[L - 4:L])
    word = int.from_bytes(wb, "big")
    index = word & 0x7FFFFFFF
    delta = i32(index - c.recv)
    if not (delta > 0 or (-delta <= 64 and not ((c.window & M64) >> ((-delta) & 63)) & 1)):
        return 1, L
    end = L - T - 4
    tag = bytes(buf[end:end + T])
    iv = rtcp_iv(c.salt, ssrc, index)
    if word & 0x80000000:
        pt = open_(c.rks, iv, bytes(buf[:8]) + wb, bytes(buf[8:end]), tag)
        if pt is None:
            return 2, end
        buf[8:end] = pt
    elif open_(c.rks, iv, bytes(buf[:end]) + wb, b"", tag) is None:
        return 2, end
    d2 = i32(c.recv - index)
    if d2 > 0:
        c.window = lshl(c.window, d2) | 1
    else:
        c.window = i64(c.window | ishl1(d2))
    c.recv = index
    return 0, end


def process(ts, reverse, seg, off, length, cap, flags=None, abort_on_error=True):
    """pyref.process's contract (numpy arrays, in place); returns the statuses."""
    n = len(off)
    status = [0] * n
    aborted = set()
    for i in range(n):
        t = ts[i] if isinstance(ts, (list, tuple)) else ts
        fl = int(flags[i]) if flags is not None else 0
        if t is None or fl & 0x80000000:
            status[i] = 9
            continue
        if id(t) in aborted:
            status[i] = 8
            continue
        o, cp = int(off[i]), int(cap[i])
        buf = bytearray(seg[o:o + cp].tobytes())
        st, L = process_one(t, reverse, buf, int(length[i]), cp, fl)
        seg[o:o + cp] = list(buf[:cp])
        length[i] = L
        status[i] = st
        if st == 6 and abort_on_error:
            aborted.add(id(t))
    return np.array(status, np.int32)


# ---------------------------------------------------------------- OpenSSL pin
_ssl = [False]


def _libcrypto():
    if _ssl[0] is False:
        _ssl[0] = None
        for name in ("libcrypto.so.3", ctypes.util.find_library("crypto")):
            try:
                if name:
                    lib = C.CDLL(name)
                    lib.EVP_aes_128_gcm.restype = lib.EVP_aes_256_gcm.restype = C.c_void_p
                    lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
                    _ssl[0] = lib
                    break
            except (OSError, AttributeError):
                continue
    return _ssl[0]


def have_openssl() -> bool:
    return _libcrypto() is not None


def openssl_gcm(key: bytes, iv: bytes, aad: bytes, data: bytes, tag: bytes = None):
    """EVP AES-GCM: seal -> (ciphertext, tag); with ``tag``: open -> plaintext
    or None on a mismatch."""
    lib = _libcrypto()
    vp = C.c_void_p
    ctx = vp(lib.EVP_CIPHER_CTX_new())
    try:
        cipher = vp(lib.EVP_aes_128_gcm() if len(key) == 16 else lib.EVP_aes_256_gcm())
        enc = 0 if tag is not None else 1
        ok = lib.EVP_CipherInit_ex(ctx, cipher, None, None, None, enc)
        ok &= lib.EVP_CIPHER_CTX_ctrl(ctx, 0x9, len(iv), None)  # EVP_CTRL_AEAD_SET_IVLEN
        ok &= lib.EVP_CipherInit_ex(ctx, None, None, bytes(key), bytes(iv), enc)
        assert ok == 1
        n = C.c_int(0)
        if aad:
            assert lib.EVP_CipherUpdate(ctx, None, C.byref(n), bytes(aad), len(aad)) == 1
        out = C.create_string_buffer(len(data) + 16)
        if data:
            assert lib.EVP_CipherUpdate(ctx, out, C.byref(n), bytes(data), len(data)) == 1
        res = out.raw[:len(data)]
        fin = C.create_string_buffer(16)
        if tag is not None:
            assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, bytes(tag)) == 1  # EVP_CTRL_AEAD_SET_TAG
            return res if lib.EVP_CipherFinal_ex(ctx, fin, C.byref(n)) == 1 else None
        assert lib.EVP_CipherFinal_ex(ctx, fin, C.byref(n)) == 1
        t = C.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, t) == 1  # EVP_CTRL_AEAD_GET_TAG
        return res, t.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


# ------------------------------------------------------------- packet helpers
def rtp_packet(ssrc: int, seq: int, payload: bytes, csrcs: int = 0, ext_words: int = -1, pt: int = 96) -> bytes:
    """An RTP packet: `csrcs` CSRC words, and with ext_words >= 0 a header
    extension of that many 4-byte words after its own 4-byte header."""
    b0 = 0x80 | csrcs | (0x10 if ext_words >= 0 else 0)
    hdr = bytes([b0, pt]) + seq.to_bytes(2, "big") + (seq * 160 & M32).to_bytes(4, "big") + ssrc.to_bytes(4, "big")
    hdr += b"".join((0xC5C00000 + i).to_bytes(4, "big") for i in range(csrcs))
    if ext_words >= 0:
        hdr += b"\xbe\xde" + ext_words.to_bytes(2, "big") + bytes((7 * i + 1) & 0xFF for i in range(4 * ext_words))
    return hdr + bytes(payload)


def rtcp_packet(ssrc: int, body: bytes) -> bytes:
    n = 8 + len(body)
    return bytes([0x80, 200]) + ((n + 3) // 4 - 1).to_bytes(2, "big") + ssrc.to_bytes(4, "big") + bytes(body)


def pack(pkts, room: int = 20, caps=None):
    """(seg, off, length, cap) of packets laid out in 16-byte aligned regions of
    len + room bytes (or caps[i])."""
    n = len(pkts)
    length = np.array([len(p) for p in pkts], np.uint32)
    cap = np.array([len(p) + room for p in pkts] if caps is None else caps, np.uint32)
    off = np.zeros(n, np.uint32)
    pos = 0
    for i in range(n):
        off[i] = pos
        pos += (int(cap[i]) + 15) & ~15
    seg = np.zeros(max(pos, 16), np.uint8)
    for i, p in enumerate(pkts):
        k = min(len(p), (int(cap[i]) + 15) & ~15)
        seg[off[i]:off[i] + k] = np.frombuffer(bytes(p[:k]), np.uint8)
    return seg, off, length, cap


def payload(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
