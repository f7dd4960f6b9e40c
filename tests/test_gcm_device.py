"""The stateless AES-GCM batch on the GPU (srtp_aes_gcm_device / k_gcm_aead):
GHASH by Shoup's 4-bit tables in LDS plus AES-CTR from the T-table image, a
lane per packet, with no parse, sort or walk around it.  Bit-exact against the
host AEAD (srtp_aes_gcm) and the test-side reference (gcm_ref), which
test_gcm_host.py pins to OpenSSL."""
import numpy as np
import pytest

import gcm_ref as G
from libjitsi_amd import _native as N
from libjitsi_amd import srtp
from test_gcm_host import KATS

pytestmark = pytest.mark.gpu

ALENS = (0, 8, 12, 16, 28, 33)
DLENS = (0, 1, 15, 16, 17, 31, 32, 33, 1188)
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(device=0, max_contexts=1024, max_factories=4, max_transformers=4)


_cases = {}


def cases(klen):
    """The 54 packets (every AAD length x every data length) of one key, with
    their sealed form from the host AEAD, checked against gcm_ref once."""
    if klen not in _cases:
        rng = np.random.default_rng(7714 + klen)
        key = rng.bytes(klen)
        rks = G.expand_key(key)
        pk = []
        for alen in ALENS:
            for dlen in DLENS:
                iv, aad, data = rng.bytes(12), rng.bytes(alen), rng.bytes(dlen)
                c, t = srtp.aes_gcm(key, iv, aad, data)
                assert G.seal(rks, iv, aad, data) == (c, t)
                pk.append((iv, aad, data, c, t))
        assert len(pk) == 54
        _cases[klen] = (key, pk)
    return _cases[klen]


class Batch:
    """n packets (the 54 cases, repeated) laid out in one segment with guard
    bytes around every packet.  aligned: every packet starts on a 16-byte
    boundary; else the packets start at odd offsets."""

    def __init__(self, klen, n, aligned, sealed):
        self.key, pk = cases(klen)
        self.pk = [pk[i % len(pk)] for i in range(n)]
        self.n = n
        off, pos = [], 16
        for iv, aad, data, c, t in self.pk:
            if aligned:
                pos = (pos + 15) & ~15
            else:
                pos |= 1
            off.append(pos)
            pos += len(aad) + len(data) + 5
        self.off = np.array(off, np.uint32)
        self.alen = np.array([len(p[1]) for p in self.pk], np.uint32)
        self.dlen = np.array([len(p[2]) for p in self.pk], np.uint32)
        self.size = pos + 16
        self.iv = np.frombuffer(b"".join(p[0] for p in self.pk), np.uint8).copy()
        self.seg = self.image(sealed)
        self.tag = self.tags() if sealed else np.full(16 * n, GUARD, np.uint8)

    def image(self, sealed):
        seg = np.full(self.size, GUARD, np.uint8)
        for o, (iv, aad, data, c, t) in zip(self.off, self.pk):
            b = aad + (c if sealed else data)
            seg[o:o + len(b)] = np.frombuffer(b, np.uint8)
        return seg

    def tags(self):
        return np.frombuffer(b"".join(p[4] for p in self.pk), np.uint8).copy()

    def data_of(self, seg, i):
        o = int(self.off[i]) + int(self.alen[i])
        return seg[o:o + int(self.dlen[i])].tobytes()


def run(eng, key, seg, off, alen, dlen, iv, tag, open_):
    """One srtp.aes_gcm_device call on copies of the host arrays; returns the
    segment, tags and results as host arrays."""
    import torch
    dev = "cuda:0"
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)  # noqa: E731
    dseg, dtag, div = d(seg, np.uint8), d(tag, np.uint8), d(iv, np.uint8)
    doff, dal, ddl = d(off, np.int32), d(alen, np.int32), d(dlen, np.int32)
    n = len(off)
    res = torch.full((n,), -7, dtype=torch.int32, device=dev)
    srtp.aes_gcm_device(eng, key, dseg, doff, dal, ddl, div, dtag, result=res, open=open_)
    torch.cuda.synchronize()
    return dseg.cpu().numpy(), dtag.cpu().numpy(), res.cpu().numpy()


SHAPES = [(klen, n, aligned) for klen in (16, 32) for n, aligned in ((54, True), (130, True), (130, False))]


@pytest.mark.parametrize("klen,n,aligned", SHAPES)
def test_seal_and_open(eng, klen, n, aligned):
    """Seal gives the host AEAD's (= gcm_ref's) ciphertext and tags and leaves
    every byte outside the packets alone; open gives the plaintext back.  130
    packets cross two wave boundaries; the unaligned layout takes the byte-wise
    loads and stores."""
    b = Batch(klen, n, aligned, sealed=False)
    seg, tag, res = run(eng, b.key, b.seg, b.off, b.alen, b.dlen, b.iv, b.tag, False)
    assert np.array_equal(seg, b.image(True))
    assert np.array_equal(tag, b.tags())
    assert (res == -7).all()  # seal does not write results
    seg2, tag2, res2 = run(eng, b.key, seg, b.off, b.alen, b.dlen, b.iv, tag, True)
    assert (res2 == 0).all()
    assert np.array_equal(seg2, b.seg)
    assert np.array_equal(tag2, tag)


@pytest.mark.parametrize("klen,n,aligned", [(16, 130, True), (32, 130, False)])
def test_one_flipped_bit_is_refused(eng, klen, n, aligned):
    """One flipped bit in a packet's tag, AAD or data: result 1 and the data
    bytes unchanged; every other packet of the batch opens as before."""
    b = Batch(klen, n, aligned, sealed=True)
    rng = np.random.default_rng(klen)
    seg, tag = b.seg.copy(), b.tag.copy()
    bad = {}
    with_aad = [i for i in range(n) if b.alen[i]]
    with_data = [i for i in range(n) if b.dlen[i]]
    for i in rng.choice(n, 9, replace=False):
        bad[int(i)] = "tag"
    for i in rng.choice(with_aad, 9, replace=False):
        bad.setdefault(int(i), "aad")
    for i in rng.choice(with_data, 9, replace=False):
        bad.setdefault(int(i), "data")
    # the last packet of the first wave and the first of the second, too
    bad.setdefault(63, "tag")
    bad.setdefault(64, "tag")
    assert {"tag", "aad", "data"} <= set(bad.values())
    for i, what in bad.items():
        bit = int(rng.integers(0, 1 << 16))
        if what == "tag":
            tag[16 * i + (bit // 8) % 16] ^= 1 << (bit % 8)
        else:
            o = int(b.off[i]) + (int(b.alen[i]) if what == "data" else 0)
            m = int(b.dlen[i]) if what == "data" else int(b.alen[i])
            seg[o + (bit // 8) % m] ^= 1 << (bit % 8)
    want = seg.copy()
    plain = b.image(False)
    for i in range(n):
        if i not in bad:
            o = int(b.off[i])
            m = int(b.alen[i]) + int(b.dlen[i])
            want[o:o + m] = plain[o:o + m]
    seg2, tag2, res = run(eng, b.key, seg, b.off, b.alen, b.dlen, b.iv, tag, True)
    assert res.tolist() == [1 if i in bad else 0 for i in range(n)]
    assert np.array_equal(seg2, want)
    assert np.array_equal(tag2, tag)


@pytest.mark.parametrize("key,pt,ct,tag", KATS)
def test_known_answers(eng, key, pt, ct, tag):
    off, alen, dlen = (np.array([v], np.uint32) for v in (16, 0, len(pt)))
    seg = np.zeros(48, np.uint8)
    seg[16:16 + len(pt)] = np.frombuffer(pt, np.uint8)
    iv = np.zeros(12, np.uint8)
    s, t, _ = run(eng, key, seg, off, alen, dlen, iv, np.zeros(16, np.uint8), False)
    assert (s[16:16 + len(pt)].tobytes().hex(), t.tobytes().hex()) == (ct, tag)
    assert not s[:16].any() and not s[16 + len(pt):].any()
    s2, _, res = run(eng, key, s, off, alen, dlen, iv, t, True)
    assert res.tolist() == [0] and s2[16:16 + len(pt)].tobytes() == pt


def test_argument_checks(eng):
    """n = 0 is SRTP_OK whatever the arrays are (nothing is launched, so NULL
    arrays are never touched); a 24-byte key, a missing key or a NULL array is
    SRTP_EINVAL."""
    import torch
    L = N.lib()
    f = L.srtp_aes_gcm_device
    assert f(eng.h, 0, bytes(16), 16, None, None, None, None, None, None, None, 0, None) == 0
    assert f(eng.h, 1, bytes(32), 32, None, None, None, None, None, None, None, 0, None) == 0
    assert f(eng.h, 0, bytes(24), 24, None, None, None, None, None, None, None, 0, None) == -1
    assert f(eng.h, 0, None, 16, None, None, None, None, None, None, None, 0, None) == -1
    assert f(None, 0, bytes(16), 16, None, None, None, None, None, None, None, 0, None) == -1
    t = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    w = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    p, q = t.data_ptr(), w.data_ptr()
    assert f(eng.h, 0, bytes(24), 24, p, q, q, q, p, p, q, 1, None) == -1
    assert f(eng.h, 0, bytes(16), 16, None, q, q, q, p, p, q, 1, None) == -1
    assert f(eng.h, 1, bytes(16), 16, p, q, q, q, p, p, None, 1, None) == -1  # open needs result
    torch.cuda.synchronize()
    assert not t.any().item() and not w.any().item()
    with pytest.raises(N.SrtpError):
        srtp.aes_gcm_device(eng, bytes(24), t, w, w, w, t, t, result=w, n=1)
    with pytest.raises(ValueError):  # int64 lengths are not the ABI's uint32
        srtp.aes_gcm_device(eng, bytes(16), t, w.to(torch.int64), w, w, t, t, n=1)
