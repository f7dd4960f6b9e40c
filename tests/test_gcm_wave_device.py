"""The stateless AES-GCM batch with a wave per packet (srtp_aes_gcm_device_ex
with SRTP_GCM_BATCH_WAVE / k_gcm_aead_wave): GHASH as a sum over the powers of
H, a block per lane, 64 blocks a chunk, and the AES-CTR blocks spread over the
lanes in steps of 128 counters.  Bit-exact against the host AEAD
(srtp_aes_gcm) and against the lane-per-packet batch (wave=False), with guard
bytes around every packet."""
import numpy as np
import pytest

from libjitsi_amd import _native as N
from libjitsi_amd import srtp
from test_gcm_host import KATS

pytestmark = pytest.mark.gpu

# the list of GHASH blocks crosses 64 with a one-block AAD at 16 * 62 data bytes;
# lane 0's second counter pair begins at data block 63 (1008 bytes); a second
# step of 128 counters at data block 127 (2032 bytes)
DLENS = (0, 1, 15, 16, 17, 31, 32, 33) + tuple(range(16 * 61 - 1, 16 * 63 + 2)) + \
    (2031, 2032, 2033, 2048, 2049, 4100)
ALENS = (0, 1, 12, 16, 17, 28, 1030)  # 1030: more than one chunk of AAD
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(device=0, max_contexts=1024, max_factories=4, max_transformers=4)


_cases = {}


def cases(klen):
    """Every AAD length x every data length under one key, sealed by the host AEAD."""
    if klen not in _cases:
        rng = np.random.default_rng(7714 + klen)
        key = rng.bytes(klen)
        pk = []
        for alen in ALENS:
            for dlen in DLENS:
                iv, aad, data = rng.bytes(12), rng.bytes(alen), rng.bytes(dlen)
                c, t = srtp.aes_gcm(key, iv, aad, data)
                pk.append((iv, aad, data, c, t))
        _cases[klen] = (key, pk)
    return _cases[klen]


class Batch:
    """Packets laid out in one segment with guard bytes around every packet.
    aligned: every packet starts on a 16-byte boundary; else at odd offsets."""

    def __init__(self, klen, picks, aligned, sealed):
        self.key, pk = cases(klen)
        self.pk = [pk[i % len(pk)] for i in picks]
        self.n = len(self.pk)
        off, pos = [], 16
        for iv, aad, data, c, t in self.pk:
            pos = (pos + 15) & ~15 if aligned else pos | 1
            off.append(pos)
            pos += len(aad) + len(data) + 5
        self.off = np.array(off, np.uint32)
        self.alen = np.array([len(p[1]) for p in self.pk], np.uint32)
        self.dlen = np.array([len(p[2]) for p in self.pk], np.uint32)
        self.size = pos + 16
        self.iv = np.frombuffer(b"".join(p[0] for p in self.pk), np.uint8).copy()
        self.seg = self.image(sealed)
        self.tag = self.tags() if sealed else np.full(16 * self.n, GUARD, np.uint8)

    def image(self, sealed):
        seg = np.full(self.size, GUARD, np.uint8)
        for o, (iv, aad, data, c, t) in zip(self.off, self.pk):
            b = aad + (c if sealed else data)
            seg[o:o + len(b)] = np.frombuffer(b, np.uint8)
        return seg

    def tags(self):
        return np.frombuffer(b"".join(p[4] for p in self.pk), np.uint8).copy()


def run(eng, key, seg, off, alen, dlen, iv, tag, open_, wave=True):
    import torch
    dev = "cuda:0"
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)  # noqa: E731
    dseg, dtag, div = d(seg, np.uint8), d(tag, np.uint8), d(iv, np.uint8)
    doff, dal, ddl = d(off, np.int32), d(alen, np.int32), d(dlen, np.int32)
    res = torch.full((len(off),), -7, dtype=torch.int32, device=dev)
    srtp.aes_gcm_device(eng, key, dseg, doff, dal, ddl, div, dtag, result=res, open=open_, wave=wave)
    torch.cuda.synchronize()
    return dseg.cpu().numpy(), dtag.cpu().numpy(), res.cpu().numpy()


def check_seal_and_open(eng, b):
    for wave in (True, False):  # the host AEAD's bytes from both kernels: so they agree with each other
        seg, tag, res = run(eng, b.key, b.seg, b.off, b.alen, b.dlen, b.iv, b.tag, False, wave)
        assert np.array_equal(tag, b.tags()), wave
        assert np.array_equal(seg, b.image(True)), wave  # every guard byte included
        assert (res == -7).all()  # seal does not write results
        seg2, tag2, res2 = run(eng, b.key, seg, b.off, b.alen, b.dlen, b.iv, tag, True, wave)
        assert (res2 == 0).all(), wave
        assert np.array_equal(seg2, b.seg), wave
        assert np.array_equal(tag2, tag), wave


N_ALL = len(ALENS) * len(DLENS)


@pytest.mark.parametrize("klen", (16, 32))
@pytest.mark.parametrize("aligned", (True, False))
def test_every_length(eng, klen, aligned):
    """Every AAD length x every data length in one batch (4 does not divide it)."""
    assert N_ALL % 4
    check_seal_and_open(eng, Batch(klen, range(N_ALL), aligned, sealed=False))


@pytest.mark.parametrize("n", (1, 3, 5, 130))
@pytest.mark.parametrize("klen,aligned", ((16, False), (32, True)))
def test_batch_sizes(eng, n, klen, aligned):
    """1, 3 and 5 packets leave waves of the last workgroup without a packet;
    130 is many workgroups.  The picks stride through the case table so that
    every AAD length and the long data lengths appear."""
    picks = [(i * 37 + 11 * n) % N_ALL for i in range(n)]
    check_seal_and_open(eng, Batch(klen, picks, aligned, sealed=False))


@pytest.mark.parametrize("klen,aligned", ((16, True), (32, False)))
def test_one_flipped_bit_is_refused(eng, klen, aligned):
    """One flipped bit in a packet's tag, AAD or data: result 1 and the data
    bytes unchanged; every other packet of the batch opens as before."""
    n = 130
    picks = [(i * 37) % N_ALL for i in range(n)]
    b = Batch(klen, picks, aligned, sealed=True)
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
    assert {"tag", "aad", "data"} <= set(bad.values())
    for i, what in bad.items():
        bit = int(rng.integers(0, 1 << 20))
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
    """gcm_batch_check's rules under the flag are srtp_aes_gcm_device's, and an
    unknown flag bit is SRTP_EINVAL."""
    import torch
    L = N.lib()
    W = N.GCM_BATCH_WAVE

    def f(*a):
        return L.srtp_aes_gcm_device_ex(*a[:-1], W, a[-1])

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
    assert L.srtp_aes_gcm_device_ex(eng.h, 0, bytes(16), 16, p, q, q, q, p, p, q, 1, 2, None) == -1
    assert L.srtp_aes_gcm_device_ex(eng.h, 0, bytes(16), 16, p, q, q, q, p, p, q, 1, W | 4, None) == -1
    torch.cuda.synchronize()
    assert not t.any().item() and not w.any().item()
    with pytest.raises(N.SrtpError):
        srtp.aes_gcm_device(eng, bytes(24), t, w, w, w, t, t, result=w, n=1, wave=True)
