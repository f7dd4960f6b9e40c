"""What of the FEC recovery (srtp_fec_recover_device / _host, k_fec_recover) can
be held without a GPU: the entry points and the record's layout, the rule
(libjitsi_amd/csrc/fec_rx_job.h through srtp_fec_recover_job) against
FECReceiver.Reconstructor restated (tests/fec_rx_ref.py), fec_rx_ref itself by
hand, the wrap quirk, the sanitizer check program, the grids the GPU tests run,
and the Python mirror's calls."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fec_ref as F
import fec_rx_grids as G
import fec_rx_ref as R
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fec_recover_device", "srtp_fec_recover_host", "srtp_fec_recover_job", "srtp_engine_fec_recover_stats")
FIELDS = ["fec", "first", "ssrc", "count", "on", "reserved"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct \{ int32_t fec; uint32_t first, ssrc; uint8_t count, on; uint16_t reserved; \} "
                     r"srtp_fec_recover;", text)
    assert [n for n, _ in N.FecRecover._fields_] == FIELDS
    offsets = [0, 4, 8, 12, 13, 14]
    assert C.sizeof(N.FecRecover) == 16 and [getattr(N.FecRecover, n).offset for n in FIELDS] == offsets
    dt = N.FEC_RECOVER_DTYPE
    assert dt.itemsize == 16 and list(dt.names) == FIELDS and [dt.fields[n][1] for n in FIELDS] == offsets
    assert dt == G._dtype()
    a = np.zeros(1, dt)
    a[0] = (-2, 0x01020304, 0xA1B2C3D4, 64, 1, 0xBEEF)
    assert a.tobytes() == bytes([0xFE, 0xFF, 0xFF, 0xFF, 4, 3, 2, 1, 0xD4, 0xC3, 0xB2, 0xA1, 64, 1, 0xEF, 0xBE])
    r = N.FecRecover.from_buffer_copy(a.tobytes())
    assert (r.fec, r.first, r.ssrc, r.count, r.on, r.reserved) == (-2, 0x01020304, 0xA1B2C3D4, 64, 1, 0xBEEF)
    for name, value in (("OFF", N.FECRX_OFF), ("RECOVERED", N.FECRX_RECOVERED), ("COMPLETE", N.FECRX_COMPLETE),
                        ("WAIT", N.FECRX_WAIT), ("PARTIAL", N.FECRX_PARTIAL)):
        assert int(re.search(r"#define SRTP_FECRX_%s (\d+)" % name, header).group(1)) == value
        assert getattr(R, name) == value
    assert re.search(r"#define SRTP_FECRX_REFUSED \(-1\)", header) and N.FECRX_REFUSED == -1 == R.REFUSED
    assert N.FECRX_MAX_CANDIDATES == 64 == R.MEDIA_BUF_SIZE
    L = N.lib()
    for name in ENTRY:
        proto = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        decl = [a.strip() for a in proto.split(",")]
        types = getattr(L, name).argtypes
        assert len(types) == len(decl), name
        for d, t in zip(decl, types):
            if "*" in d:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, d, t)
            else:
                want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "size_t": C.c_size_t}[d.split()[0]]
                assert t is want, (name, d, t)
    names = ["calls", "records", "recovered", "complete", "waiting", "partial", "refused", "member_bytes"]
    assert [n for n, _ in N.FecRecoverStats._fields_] == names and C.sizeof(N.FecRecoverStats) == 64
    assert re.search(r"uint64_t %s;\s*\} srtp_fec_recover_stats;" % ", ".join(names), text)
    assert "fec_rx_job.h" in N.KERNEL_SOURCES


@pytest.mark.parametrize("n_rec", [0, 1])
def test_null_engine_is_einval(n_rec):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    rec = (N.FecRecover * 4)()
    out = (C.c_int8 * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fec_recover_device(None, p(buf), p(w), p(w), p(w), None, 1, p(rec), n_rec, p(i), 4, p(buf), p(w),
                                     p(w), p(w), p(i), p(out), None) == -1
    assert L.srtp_fec_recover_host(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(rec), n_rec, p(i), 4, p(buf), 64,
                                   p(w), p(w), p(w), p(i), p(out)) == -1
    assert L.srtp_engine_fec_recover_stats(None, C.byref(N.FecRecoverStats())) == -1
    ln, code = C.c_int32(7), C.c_int8(7)
    assert L.srtp_fec_recover_job(None, p(buf), 64, p(buf), p(w), p(w), p(buf), 64, C.byref(ln), C.byref(code)) == -1
    assert L.srtp_fec_recover_job(rec, p(buf), 64, p(buf), p(w), p(w), p(buf), 64, None, C.byref(code)) == -1
    assert (ln.value, code.value) == (7, 7)
    rec[0].on, rec[0].count = 1, 1
    assert L.srtp_fec_recover_job(rec, None, 64, p(buf), p(w), p(w), p(buf), 64, C.byref(ln), C.byref(code)) == -1
    rec[0].on = 0
    assert L.srtp_fec_recover_job(rec, None, 0, None, None, None, None, 0, C.byref(ln), C.byref(code)) == 0  # off
    assert (ln.value, code.value) == (0, 0)


def job(fec, cands, ssrc, out_cap=None, over=None):
    """srtp_fec_recover_job over the packets: (code, len_out, bytes of the output buffer)."""
    rec = N.FecRecover(-7, 0xFFFFFFF0, ssrc, len(cands), 1, 0xBEEF)  # fec and first are not read
    for k, v in (over or {}).items():
        setattr(rec, k, v)
    blob = b"".join(cands) or b"\0"
    at = np.cumsum([0] + [len(m) for m in cands[:-1]]).astype(np.uint32) if cands else np.zeros(1, np.uint32)
    lens = np.array([len(m) for m in cands] or [0], np.uint32)
    cap = len(fec) + 40 if out_cap is None else out_cap
    out = (C.c_uint8 * max(cap, 1))(*([0xEE] * max(cap, 1)))
    ln, code = C.c_int32(), C.c_int8()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    fb = (C.c_uint8 * max(len(fec), 1)).from_buffer_copy(fec or b"\0")
    assert N.lib().srtp_fec_recover_job(C.byref(rec), C.cast(fb, C.c_void_p), len(fec), C.cast(buf, C.c_void_p),
                                        at.ctypes.data, lens.ctypes.data, C.cast(out, C.c_void_p), cap, C.byref(ln),
                                        C.byref(code)) == 0
    return code.value, ln.value, bytes(out)


def agree(fec, cands, ssrc, note):
    """The job against the reference, into regions roomy, exact and one byte short."""
    want_code, want = R.one(fec, cands, ssrc)
    code, ln, out = job(fec, cands, ssrc)
    assert code == want_code and ln == (len(want) if want else 0), note
    if want is None:
        assert set(out) == {0xEE}, note
        return code
    assert out[:ln] == want and set(out[ln:]) <= {0xEE}, note
    code, ln, out = job(fec, cands, ssrc, out_cap=len(want))
    assert (code, ln) == (1, len(want)) and out == want, note
    code, ln, out = job(fec, cands, ssrc, out_cap=len(want) - 1)
    assert (code, ln) == (1, len(want)) and out == want[:-1], note
    return code


SINGLE = (12, 13, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1200, 2036)


def test_recover_job_agrees_with_the_reference():
    """Needed counts 0, 1, 3, 4, 5, 15, 16 and 47, member lengths around every piece boundary alone and mixed,
    header lengths 12 / 16 / 20 / 24, both masks, a recovered length above and below every member's, output
    regions one byte short, exact and roomy; groups made by fec_ref.make and hand-built ones."""
    rng = np.random.default_rng(5109)
    cases = 0
    for needed in (0, 1, 3, 4, 5, 15, 16, 47):
        count = needed + 1
        for t, n in enumerate(SINGLE):
            base = int(rng.integers(0, 65000))
            for mixed in (False, True):
                lens = [int(rng.integers(12, n + 1)) for _ in range(count)] if mixed else [n] * count
                lost = int(rng.integers(0, count))
                if mixed:
                    lens[lost] = n if t % 2 else 12  # above, or below, every other member's
                media = [G.packet(rng, base + k, c) for k, c in enumerate(lens)]
                others = [m for i, m in enumerate(media) if i != lost]
                rng.shuffle(others)
                extra = [G.packet(rng, base - 1 - k, 12 + k) for k in range(int(rng.integers(0, 64 - needed)))]
                hl = (12, 16, 20, 24)[(t + needed) % 4]
                long_mask = count > 16 or bool((t + mixed) % 2)
                fec = G.make_fec(rng, media, list(range(count)), base, hl, long_mask)
                ssrc = int(rng.integers(0, 1 << 32))
                assert agree(fec, extra + others, ssrc, (needed, lens, hl, long_mask)) == R.RECOVERED
                got = R.one(fec, others, ssrc)[1]
                assert got[:8] == media[lost][:8] and got[12:] == media[lost][12:] and got[8:12] == ssrc.to_bytes(4, "big")
                if count <= 16:  # what the sender makes
                    sent = F.make(media, 77, 116)
                    assert agree(sent, others + extra, ssrc, (needed, lens, "sender")) == R.RECOVERED
                    assert R.one(sent, others, ssrc)[1] == got
                assert agree(fec, media, ssrc, "complete") == R.COMPLETE
                if count >= 2:
                    assert agree(fec, others[1:], ssrc, "wait") == R.WAIT
                cases += 1
    assert cases == 8 * 14 * 2
    # the record's own fields, and a FEC packet that does not count
    good = [G.packet(rng, 7 + k, 40) for k in range(3)]
    fec = F.make(good, 1, 116)
    assert job(fec, good[:2] * 32, 5)[0] == R.RECOVERED          # 64 candidates
    assert job(fec, good[:2], 5, over=dict(count=65))[:2] == (R.REFUSED, 0)
    assert job(fec[:11], good[:2], 5)[:2] == (R.REFUSED, 0)
    assert job(fec, good[:2], 5, over=dict(on=0))[:2] == (R.OFF, 0)
    assert job(fec, good[:2], 5, over=dict(on=2))[0] == R.RECOVERED  # any value but 0 is on
    # absent candidates, duplicates: the later one stands
    twin = G.packet(rng, 8, 40)
    assert agree(fec, [good[0], b"short", good[1]], 5, "absent") == R.RECOVERED
    assert agree(fec, [good[0], good[1], twin], 5, "twin behind") == R.RECOVERED
    assert agree(fec, [good[0], twin, good[1]], 5, "twin in front") == R.RECOVERED
    assert R.one(fec, [good[0], good[1], twin], 5)[1] != R.one(fec, [good[0], twin, good[1]], 5)[1]
    # partial, and every cut of the FEC packet
    part = G.make_fec(rng, [good[0], G.packet(rng, 8, 90)], [0, 1], 7, plen=40)
    assert agree(part, [good[0]], 5, "partial") == R.PARTIAL
    for hl in (12, 16, 20, 24):
        for long_mask in (False, True):
            full = G.make_fec(rng, good, [0, 1, 2], 7, hl, long_mask)
            pay = hl + (18 if long_mask else 14)
            for cut in range(0, len(full) + 1):
                code = agree(full[:cut], [good[0], good[2]], 5, (hl, long_mask, cut))
                assert code == (R.RECOVERED if cut >= pay + 28 else R.REFUSED)


def test_fec_rx_ref_by_hand():
    """One three-packet group written out, and fec_ref.recover agreeing where the SSRCs coincide."""
    a = bytes.fromhex("80e4 0010 00000100 11111111") + bytes([0x01, 0x02, 0x03, 0x04])
    b = bytes.fromhex("90e4 0011 00000200 11111111") + bytes([0x10, 0x20])
    c = bytes.fromhex("80e4 0012 00000400 11111111") + bytes([0xFF, 0x00, 0xFF, 0x00, 0xFF, 0x07])
    fec = F.make([a, b, c], 0x11111111, 0x74)
    # lost b: length 4 ^ 6 ^ (4 ^ 2 ^ 6) = 2; byte 0 = 0x90 ^ 0x80 ^ 0x80, version forced; TS = 0x700 ^ 0x100 ^ 0x400
    code, got = R.one(fec, [a, c], 0x11111111)
    assert code == R.RECOVERED
    assert got == bytes.fromhex("90e4 0011 00000200 11111111") + bytes([0x10, 0x20]) == b
    for lost, pkt in enumerate((a, b, c)):
        others = [p for i, p in enumerate((a, b, c)) if i != lost]
        code, got = R.one(fec, others, 0x11111111)
        assert code == R.RECOVERED and got == pkt == F.recover(fec, others)
        assert R.one(fec, others, 0xCAFEF00D)[1] == pkt[:8] + bytes.fromhex("cafef00d") + pkt[12:]
    assert R.one(fec, [a, b, c], 1) == (R.COMPLETE, None) and R.one(fec, [a], 1) == (R.WAIT, None)
    assert R.one(fec, [], 1) == (R.WAIT, None) and R.one(fec[:25], [a, c], 1) == (R.REFUSED, None)
    assert R.header_length(bytes.fromhex("90000000 00000000 00000000 0000 0002")) == 24
    assert R.header_length(bytes.fromhex("91000000 00000000 00000000 00000000 0000 ffff")) == 16
    assert R.header_length(bytes.fromhex("90000000 00000000 00000000 0000 00")) is None
    assert [R.seq_cmp(*p) for p in ((1, 1), (2, 1), (1, 2), (65535, 0), (0, 65535), (40000, 1))] == [0, 1, -1, -1, 1, -1]
    assert R.first_key({65534: 0, 1: 0, 65535: 0, 0: 0}) == 65534


def test_the_wrap_quirk_both_outcomes():
    """base + k is not reduced mod 2^16: a complete group with one key past 65535 recovers a duplicate of a packet
    that was received, with two such keys it waits for ever.  Reference and rule alike."""
    rng = np.random.default_rng(65535)
    media = [G.packet(rng, 65533 + k, 40 + k) for k in range(4)]
    assert [R.seq_of(m) for m in media] == [65533, 65534, 65535, 0]
    one_past = F.make(media, 9, 116)
    assert agree(one_past, media, 9, "one key past the wrap") == R.RECOVERED
    got = R.one(one_past, media, 9)[1]
    assert R.seq_of(got) == 0 and got[12:] == media[3][12:] and len(got) == len(media[3])  # packet 0, again
    assert agree(one_past, media[:3], 9, "the same without it") == R.RECOVERED
    assert agree(one_past, [media[0], media[1], media[3]], 9, "one truly lost") == R.WAIT
    later = [G.packet(rng, 65534 + k, 40 + k) for k in range(4)]
    two_past = F.make(later, 9, 116)
    assert agree(two_past, later, 9, "two keys past the wrap") == R.WAIT
    before = [G.packet(rng, 65532 + k, 40 + k) for k in range(4)]
    assert agree(F.make(before, 9, 116), before, 9, "none past the wrap") == R.COMPLETE


def test_fec_recover_check_builds_and_runs_clean(tmp_path):
    """tools/fec_recover_check (the Makefile's recipe, built out of tree): a
    program of its own under AddressSanitizer + UBSan, nothing preloaded."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fec_recover_check: fec_recover_check\.cpp .*fec_rx_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fec_recover_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fec_recover_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fec_recover_check: [1-9]\d* records \([1-9]\d* recovered, [1-9]\d* complete, [1-9]\d* waiting, "
                     r"[1-9]\d* partial, [1-9]\d* refused\), [1-9]\d* pieces, [1-9]\d* refusal checks, 0 failures",
                     r.stdout)


@pytest.mark.parametrize("name", sorted(G.ALL))
def test_every_gpu_grid_holds_every_code(name):
    """By fec_rx_ref alone: each grid of tests/test_fec_recover.py holds every code it claims, in the counts the
    GPU tests assert; and the rule (srtp_fec_recover_job) agrees with the reference on every record of it."""
    g = G.ALL[name]()
    got = G.counts(g)
    assert got == G.COUNTS[name]
    assert got[0] <= 400 and got[0] == sum(got[1:])
    if name != "all_refused":
        assert all(c > 0 for c in got[1:])
    else:
        assert got[1:5] == (0, 0, 0, 0) and got[5] > 0 and got[6] > 0
    rec, cand, out_off, out_cap, out_bytes = G.arrays(g)
    assert len(rec) == got[0] and (out_off % 16 == 0).all() and int(out_off[-1]) + G.up16(int(out_cap[-1])) <= out_bytes
    want = G.expect(g)
    for r, (x, w) in enumerate(zip(g["records"], want)):
        if G.field_causes(g, r):
            continue
        first, count = int(rec["first"][r]), int(rec["count"][r])
        assert cand[first:first + count].tolist() == [G.resolve(g, c) for c in x["cands"]]
        if not x["on"]:
            continue
        fec = G.present(g, x["fec"])
        cands = [G.present(g, c) or b"" for c in x["cands"]]
        code, ln, out = job(fec or b"", cands, x["ssrc"], out_cap=int(out_cap[r]))
        assert (code, ln) == (w[0], w[2]), (name, r)
        if w[1] is not None:
            n = min(ln, int(out_cap[r]))
            assert out[:n] == w[1][:n], (name, r)
    if name == "refusals_host":
        assert not any(G.field_causes(g, r) for r in range(len(g["records"])))
    if name == "refusals_device":
        causes = {c for r in range(len(g["records"])) for c in G.field_causes(g, r)}
        assert causes == {"count", "first + count", "fec index", "candidate index"}
    if name == "boundaries":  # regions one byte short, exact and roomy among the recovered records
        deltas = {int(out_cap[r]) - w[2] for r, w in enumerate(want) if w[0] == R.RECOVERED}
        assert {-1, 0, G.ROOM} <= deltas and sum(1 for w in want if w[3] == 7) >= 10
    if name == "mixed":
        assert max(len(x["cands"]) for x in g["records"]) == 63
        shared = [tuple(x["cands"]) for x in g["records"]]
        assert len(shared) - len(set(shared)) >= 2  # records over the same candidates


# ------------------------------------------------- the calls the Python methods make
class Recorder:
    """Stands in for the loaded library: every call is noted and answers SRTP_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class Tensor:
    def __init__(self, ptr, nbytes, item=1):
        self.ptr, self.nbytes, self.item = ptr, nbytes, item

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.nbytes // self.item

    def element_size(self):
        return self.item


def test_python_mirrors(monkeypatch):
    from libjitsi_amd import FecReceiver, SRTPEngine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fec_recover_device) == ["self", "seg", "off", "length", "cap", "status", "rec", "cand",
                                                  "out_seg", "out_off", "out_cap", "out_len", "out_status", "code",
                                                  "n", "n_rec", "n_cand", "stream"]
    assert sig(SRTPEngine.fec_recover_host) == ["self", "seg", "off", "length", "cap", "rec", "cand", "out_seg",
                                                "out_off", "out_cap", "status"]
    assert sig(FecReceiver.__init__)[:3] == ["self", "ssrc", "ulpfec_pt"]
    assert "FECReceiver" in SRTPEngine.fec_recover_device.__doc__ and ":472-520" in SRTPEngine.fec_recover_device.__doc__
    assert ":233-319" in FecReceiver.reverse_transform.__doc__ and ":472-520" in FecReceiver.__doc__
    with pytest.raises(ValueError):
        FecReceiver(1, 128)
    f = FecReceiver(0x1_0000_0001, 116)
    assert (f.ssrc, f.ulpfec_pt, f.nb_fec, f.nb_recovered) == (1, 116, 0, 0)

    lib = Recorder()
    monkeypatch.setattr(N, "lib", lambda: lib)
    eng = SRTPEngine.__new__(SRTPEngine)
    eng.h = 0x1234
    n, n_rec = 5, 2
    seg, out_seg = np.zeros(320, np.uint8), np.zeros(128, np.uint8)
    a32 = lambda k: np.zeros(k, np.uint32)
    rec, cand = np.zeros(n_rec, N.FEC_RECOVER_DTYPE), np.arange(4, dtype=np.int32)
    ol, os_, code = eng.fec_recover_host(seg, a32(n), a32(n), a32(n), rec, cand, out_seg, a32(n_rec), a32(n_rec))
    name, args = lib.calls[-1]
    assert name == "srtp_fec_recover_host" and len(args) == 19
    assert args[0] == 0x1234 and args[1] == seg.ctypes.data and args[2] == 320 and args[6] is None and args[7] == n
    assert args[9] == n_rec and args[10] is not None and args[11] == 4 and args[12] == out_seg.ctypes.data
    assert args[13] == 128 and args[16:] == (ol.ctypes.data, os_.ctypes.data, code.ctypes.data)
    assert (ol.dtype, os_.dtype, code.dtype) == (np.uint32, np.int32, np.int8) and len(code) == n_rec
    eng.fec_recover_host(seg, a32(n), a32(n), a32(n), rec, None, out_seg, a32(n_rec), a32(n_rec), status=np.zeros(n))
    assert lib.calls[-1][1][10:12] == (None, 0) and lib.calls[-1][1][6] is not None

    t = lambda ptr, nbytes, item=4: Tensor(ptr, nbytes, item)
    dev = (t(0x1000, 320, 1), t(0x2000, 4 * n), t(0x3000, 4 * n), t(0x4000, 4 * n), t(0x5000, 4 * n),
           t(0x6000, 16 * n_rec, 1), t(0x7000, 16), t(0x8000, 128, 1), t(0x9000, 4 * n_rec), t(0xA000, 4 * n_rec),
           t(0xB000, 4 * n_rec), t(0xC000, 4 * n_rec), t(0xD000, n_rec, 1))
    eng.fec_recover_device(*dev)
    name, args = lib.calls[-1]
    assert name == "srtp_fec_recover_device" and len(args) == 18
    assert args == (0x1234, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, n, 0x6000, n_rec, 0x7000, 4, 0x8000, 0x9000,
                    0xA000, 0xB000, 0xC000, 0xD000, None)
    eng.fec_recover_device(*dev[:4], None, dev[5], None, *dev[7:])
    assert lib.calls[-1][1][5] is None and lib.calls[-1][1][9:11] == (None, 0)
    calls = len(lib.calls)
    with pytest.raises(ValueError):
        eng.fec_recover_device(*dev[:5], t(0x6000, 16 * n_rec - 1, 1), *dev[6:])
    with pytest.raises(ValueError):
        eng.fec_recover_device(*dev[:12], t(0xD000, n_rec - 1, 1))
    with pytest.raises(ValueError):
        eng.fec_recover_device(*dev, n_cand=5)
    assert len(lib.calls) == calls


def test_fec_receiver_bookkeeping_and_calls():
    """FecReceiver through a stand-in engine that answers with fec_rx_ref: what it keeps, evicts, removes and
    places, the order in which it repeats the call, and the arguments it makes the call with."""
    from libjitsi_amd import FecReceiver, RawPacket
    seen = []

    class Eng:
        def fec_recover_host(self, seg, off, length, cap, rec, cand, out_seg, out_off, out_cap, status=None):
            seen.append(dict(n=len(off), rec=rec.copy(), cand=np.array(cand)))
            assert (np.asarray(off) % 16 == 0).all() and status is None and (np.asarray(cap) == np.asarray(length)).all()
            pk = [bytes(seg[int(o):int(o) + int(n)]) for o, n in zip(off, length)]
            ol, st, code = np.zeros(len(rec), np.uint32), np.full(len(rec), 9, np.int32), np.zeros(len(rec), np.int8)
            for r, x in enumerate(rec):
                cs = [pk[int(c)] for c in cand[int(x["first"]):int(x["first"]) + int(x["count"])]]
                code[r], got = R.one(pk[int(x["fec"])], cs, int(x["ssrc"]))
                if got is not None:
                    assert len(got) <= out_cap[r]
                    out_seg[int(out_off[r]):int(out_off[r]) + len(got)] = np.frombuffer(got, np.uint8)
                    ol[r], st[r] = len(got), 0
            return ol, st, code

    rng = np.random.default_rng(233)
    rp = lambda b: RawPacket(b, 0, len(b))
    mine, ref = FecReceiver(0xABCD, 116, engine=Eng()), R.FECReceiver(0xABCD, 116)
    # a cascade: A = packets 100..103 + FEC 104, B = 103, 105, 106 + FEC 107 (long mask); 101 and 103 are lost:
    # B's packet needs A's recovery first -- and A needs B's.  Neither recovers until one more arrives.
    m = {s: G.packet(rng, s, 30 + s % 7) for s in (100, 101, 102, 103, 105, 106)}
    fa = bytearray(F.make([m[100], m[101], m[102], m[103]], 0xABCD, 116))
    fb = bytearray(G.make_fec(rng, [m[103], m[105], m[106]], [0, 2, 3], 103, 12, True))
    fb[2:4] = (107).to_bytes(2, "big")
    fa, fb = bytes(fa), bytes(fb)
    batch = [m[100], None, m[102], fa, m[105], m[106], fb]
    got = mine.reverse_transform([None if b is None else rp(b) for b in batch])
    want = ref.reverse_transform(batch)
    data = lambda ps: [None if p is None else p.data() for p in ps]
    assert data(got) == want and want[1] == m[103][:8] + bytes.fromhex("0000abcd") + m[103][12:]
    # in order: FEC 104 lacks two and waits, FEC 107 recovers 103; the reference does not go back to 104 in this call
    assert (mine.nb_fec, mine.nb_recovered) == (2, 1) == (ref.nb_fec, ref.nb_recovered)
    assert sorted(mine.fec) == [104] == sorted(ref.fecs) and sorted(mine.media) == sorted(ref.media)
    assert [len(c["rec"]) for c in seen] == [2] and seen[0]["n"] == 4 + 2
    assert seen[0]["rec"]["fec"].tolist() == [4, 5] and seen[0]["rec"]["count"].tolist() == [4, 4]
    assert seen[0]["rec"]["on"].tolist() == [1, 1] and seen[0]["cand"].tolist() == [0, 1, 2, 3]
    assert set(seen[0]["rec"]["ssrc"].tolist()) == {0xABCD}
    # the next call: nothing new but FEC 104 now lacks one
    del seen[:]
    got = mine.reverse_transform([None, None])
    want = ref.reverse_transform([None, None])
    assert data(got) == want and want[0][12:] == m[101][12:] and want[1] is None
    assert mine.nb_recovered == 2 == ref.nb_recovered and not mine.fec and not ref.fecs
    # the cascade inside one call: C = 200..203 + FEC 204 lacking 201, D = 201, 205 + FEC 206 lacking 205:
    # FEC 206 is asked after FEC 204 has recovered 201, so the call is repeated once for the record behind
    m = {s: G.packet(rng, s, 40 + s % 5) for s in (200, 201, 202, 203, 205)}
    fc = F.make([m[200], m[201], m[202], m[203]], 0xABCD, 116)
    fd = bytearray(G.make_fec(rng, [m[201], m[205]], [0, 4], 201))
    fd[2:4] = (206).to_bytes(2, "big")
    batch = [bytes(fd), m[200], m[202], m[203], fc]
    del seen[:]
    got = mine.reverse_transform([rp(b) for b in batch])
    want = ref.reverse_transform(batch)
    assert data(got) == want and [R.seq_of(p) for p in want] == [201, 200, 202, 203, 205]
    assert [c["rec"]["fec"].tolist() for c in seen] == [[seen[0]["n"] - 2, seen[0]["n"] - 1], [seen[1]["n"] - 1]]
    assert seen[1]["n"] == seen[0]["n"]  # one media packet more, one FEC packet less
    assert mine.nb_recovered == 4 == ref.nb_recovered and not mine.fec
    # a recovered packet is appended where no slot is empty; a complete group's FEC packet is dropped
    m2 = [G.packet(rng, 300 + k, 50) for k in range(3)]
    f2 = bytearray(F.make(m2, 1, 116))
    f2[2:4] = (303).to_bytes(2, "big")
    assert data(mine.reverse_transform([rp(m2[0]), rp(m2[1]), rp(m2[2]), rp(bytes(f2))])) == \
        ref.reverse_transform([m2[0], m2[1], m2[2], bytes(f2)])
    assert not mine.fec and not ref.fecs
    # eviction: the media map holds 64, the FEC map 32, the oldest under the comparator goes, across the wrap
    mine, ref = FecReceiver(0xABCD, 116, engine=Eng()), R.FECReceiver(0xABCD, 116)
    for k in range(80):
        s = (65500 + 3 * k) & 0xFFFF
        media = [G.packet(rng, s, 20), G.packet(rng, s + 1, 20)]
        f = bytearray(F.make(media, 1, 116))  # its sequence number: s + 2
        a = mine.reverse_transform([rp(media[0]), rp(bytes(f))])  # the second is lost, and recovered
        b = ref.reverse_transform([media[0], bytes(f)])
        assert data(a) == b and R.seq_of(b[1]) == (s + 1) & 0xFFFF
    assert len(mine.media) == 64 == len(ref.media) and sorted(mine.media) == sorted(ref.media)
    waiting = []
    for k in range(40):  # FEC packets that wait for ever: two lost each
        s = 2000 + 4 * k  # fewer than 2^15 in front of the oldest media packet kept
        media = [G.packet(rng, s + i, 20) for i in range(3)]
        f = F.make(media, 1, 116)
        waiting.append(f)
        assert data(mine.reverse_transform([rp(f)])) == ref.reverse_transform([f]) == [None]
    assert len(mine.fec) == 32 == len(ref.fecs) and sorted(mine.fec) == sorted(ref.fecs)
    assert min(mine.fec) == 2000 + 4 * 8 + 3
