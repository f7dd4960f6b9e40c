"""Fan-out that patches the payload, as seen without a GPU: the entry points and
the 8-byte record agree between the header, _native.py and the built library; a
NULL engine is refused before any device is touched; srtp_fanout_pay_job
(fanout_job.h's fanout_pay_bound and fanout_pay_piece, the text k_fanout_pay
compiles) agrees with payload_ref -- RawPacket.writeShort and rewriteFEC's two
stores restated byte by byte under the per-byte bound -- over the sweep
tools/fanout_pay_check runs; that program builds and runs clean under
AddressSanitizer + UBSan; fec_sn_bytes keeps Java's precedence; and the _ast
methods of SRTPEngine still make the C calls they made before."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import payload_ref as P
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device_pay", "srtp_fanout_host_pay", "srtp_fanout_pay_job")
SKIP = N.PKT_FLAG_SKIP
FIELDS = ["at0", "b0", "at1", "b1"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct srtp_fanout_payload \{([^{}]*)\} srtp_fanout_payload;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint16_t at0; uint8_t b0[2]; uint16_t at1; uint8_t b1[2];"
    assert [n for n, _ in N.FanoutPayload._fields_] == FIELDS
    assert C.sizeof(N.FanoutPayload) == 8
    assert [getattr(N.FanoutPayload, n).offset for n in FIELDS] == [0, 2, 4, 6]
    # pay follows stamp in both entries; the ctypes signatures have the header's argument counts and kinds
    L = N.lib()
    for name in ENTRY:
        proto = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        decl = [a.strip() for a in proto.split(",")]
        args = [a.split("*")[-1].split()[-1] for a in decl]
        types = getattr(L, name).argtypes
        assert len(types) == len(decl), name
        for d, t in zip(decl, types):
            if "*" in d:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, d, t)
            else:
                want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "size_t": C.c_size_t}[d.split()[0]]
                assert t is want, (name, d, t)
        if name != "srtp_fanout_pay_job":
            assert args[args.index("rewrite") + 1] == "stamp" and args[args.index("stamp") + 1] == "pay"
            assert args[args.index("pay") + 1] == "status"
    assert int(re.search(r"#define SRTP_MI355X_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION
    # no existing struct grew
    assert C.sizeof(N.FanoutStats) == 40 and C.sizeof(N.FanoutRewrite) == 16 and C.sizeof(N.FanoutAbsSendTime) == 8


def test_record_dtype_round_trips():
    """A numpy record and the ctypes struct are the same 8 bytes."""
    dt = N.FANOUT_PAYLOAD_DTYPE
    assert dt.itemsize == 8 and list(dt.names) == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 2, 4, 6]
    a = np.zeros(1, dt)
    a["at0"], a["b0"], a["at1"], a["b1"] = 0x1234, (0xA1, 0xA2), 0xFFEE, (0xB1, 0xB2)
    assert a.tobytes() == bytes([0x34, 0x12, 0xA1, 0xA2, 0xEE, 0xFF, 0xB1, 0xB2])
    r = N.FanoutPayload.from_buffer_copy(a.tobytes())
    assert (r.at0, list(r.b0), r.at1, list(r.b1)) == (0x1234, [0xA1, 0xA2], 0xFFEE, [0xB1, 0xB2])
    assert np.zeros(3, dt).tobytes() == bytes(24)  # an all-zero record is eight zero bytes


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    rw = (N.FanoutRewrite * 4)()
    ast = (N.FanoutAbsSendTime * 4)()
    pay = (N.FanoutPayload * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device_pay(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                    None, p(rw), p(ast), p(pay), p(i), n, None) == -1
    assert L.srtp_fanout_host_pay(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                                  p(w), None, p(rw), p(ast), p(pay), p(i), n) == -1
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert L.srtp_fanout_pay_job(0, 1, 64, 64, 0, 64, 0, None, 0, w, out) == -1
    assert L.srtp_fanout_pay_job(0, 1, 64, 64, 0, 64, 0, pay, 0, None, out) == -1
    assert L.srtp_fanout_pay_job(0, 1, 64, 64, 0, 64, 0, pay, 0, w, None) == -1
    assert L.srtp_fanout_pay_job(0, 1, 64, 64, 0, 64, 0, pay, -1, w, out) == -1
    assert list(out) == [7, 7, 7, 7]


def test_python_mirrors():
    from libjitsi_amd import SRTPEngine, fan_out_ast, fan_out_pay, fan_out_rw, fec_sn_bytes
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device_pay) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                                 "seg", "off", "length", "cap", "status", "rewrite", "stamp", "pay",
                                                 "src_status", "flags", "m", "n", "stream"]
    assert sig(SRTPEngine.fanout_host_pay) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                               "seg", "off", "cap", "src_status", "flags", "rewrite", "stamp", "pay"]
    assert sig(fan_out_pay) == ["pkts", "transformers", "rewriters", "stampers", "exclusion"]
    for f in (fan_out_pay, SRTPEngine.fanout_device_pay, SRTPEngine.fanout_host_pay):
        assert "ExtendedSequenceNumberInterval.java" in f.__doc__ and "261-284" in f.__doc__ and "346-386" in f.__doc__
    assert fan_out_pay([], [], [], []) == []
    assert fan_out_pay([None], [], [], []) == []
    with pytest.raises(ValueError):
        fan_out_pay([], [], [], [None])
    with pytest.raises(ValueError):
        fan_out_pay([], [], [None], [])
    # Java: snRewritenBase & 0xff00 >> 8 is snRewritenBase & 0xff -- both bytes are the low byte
    assert fec_sn_bytes(0x1234) == (0x34, 0x34) == P.fec_bytes(0x1234)
    assert "0xff00 >> 8" in fec_sn_bytes.__doc__ and "low byte" in fec_sn_bytes.__doc__
    for sn in (0, 1, 0xFF, 0x100, 0xABCD, 0xFFFF, 0x12345, -1):
        assert fec_sn_bytes(sn) == P.fec_bytes(sn) == (sn & 0xFF, sn & 0xFF)
    buf = bytearray(range(40))
    P.rewrite_fec(buf, 20, 0x1234)
    assert bytes(buf) == bytes(range(22)) + b"\x34\x34" + bytes(range(24, 40))
    buf = bytearray(range(40))
    P.write_short(buf, 16, 0xBEEF)
    assert bytes(buf) == bytes(range(16)) + b"\xBE\xEF" + bytes(range(18, 40))
    buf = bytearray(range(17))
    P.write_short(buf, 16, 0xBEEF)  # the per-byte bound: the first byte only
    assert bytes(buf) == bytes(range(16)) + b"\xBE"
    buf = bytearray(range(40))
    P.write_short(buf, 11, 0xBEEF)  # refused whole
    assert bytes(buf) == bytes(range(40))


# ------------------------------------------------------------------ the sweep
def sweep():
    """(src_idx, m, src_len, src_cap, src_status, dst_cap, flags, at0, at1): tools/fanout_pay_check's."""
    for c in list(range(0, 41)) + list(range(1008, 1041)) + list(range(2032, 2065)):
        few = sorted({0, 11, 12} | {c + d for d in (-2, -1, 0, 1) if c + d >= 0})
        every = sorted(set(few) | {b - 1 for b in range(16, c + 17, 16)} | {b for b in range(16, c + 17, 16)})
        for at0 in every:
            near = {at0 + d for d in (-2, -1, 0, 1, 2) if at0 + d >= 0}
            if at0 not in few and 64 < at0 < c - 64 and (at0 >> 4) % 8 not in (0, 7):
                continue  # the inner boundaries of a long copy: every eighth pair of them
            for at1 in sorted(set(few) | near):
                yield 0, 1, c, c + 40, 0, c + 40, 0, at0, at1
                if at0 in few:
                    yield 0, 1, c + 40, c + 40, 0, c, 0, at0, at1
                    yield 0, 1, c + 40, c, 0, c + 40, 0, at0, at1
        for at in few:
            yield 0, 1, c, c, 0, c, SKIP, at, at
            yield 0, 1, c, c, 2, c, 0, at, 12
            yield 1, 1, c, c, 0, c, 0, at, 12
            yield -1, 3, c, c, 0, c, 0, 12, at
            yield 0, 1, -1, c, 0, c, 0, 12, at
            yield 0, 1, c, -1, 0, c, 0, 12, at
            yield 0, 1, c, c, 0, -1, 0, 12, at
            yield 0, 1, 2 ** 31 - 1, c, 0, c + 16, 0, at, (c - 1) & 0xFFFF


SRC = bytes((7 * i + 3) & 0xFF for i in range(2128))
B0, B1 = (0xC1, 0xD2), (0xE3, 0xF4)


def test_pay_job_agrees_with_the_reference():
    job = N.lib().srtp_fanout_pay_job
    rec = N.FanoutPayload()
    rec.b0[0], rec.b0[1], rec.b1[0], rec.b1[1] = B0 + B1
    wi, wo = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    cases = patched = halves = 0
    for idx, m, L, sc, st, dc, fl, at0, at1 in sweep():
        skipped = idx < 0 or idx >= m or st != 0 or fl & SKIP
        c = 0 if skipped or min(L, sc, dc) < 0 else min(L, sc, dc, 65535)
        want = P.apply(bytearray(SRC[:c]), (at0, B0, at1, B1)) + SRC[c:]
        rec.at0, rec.at1 = at0, at1
        pieces = {0, at0 >> 4, (at0 + 1) >> 4, at1 >> 4, (at1 + 1) >> 4, max(c - 1, 0) >> 4, (c >> 4) + 1, cases % 131}
        for q in sorted(x for x in pieces if 16 * x + 16 <= len(SRC)):
            wi[:] = np.frombuffer(SRC[16 * q:16 * q + 16], "<u4").tolist()
            assert job(idx, m, L, sc, st, dc, fl, C.byref(rec), q, wi, wo) == 0
            got = np.array(list(wo), "<u4").tobytes()
            assert got == bytes(want[16 * q:16 * q + 16]), (idx, m, L, sc, st, dc, fl, at0, at1, q, got.hex())
        cases += 1
        patched += bytes(want) != SRC
        halves += (at0 >= 12 and at0 == c - 1) or (at1 >= 12 and at1 == c - 1)
    assert cases > 20000 and patched > 10000 and halves > 1000


def test_fanout_pay_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_pay_check (the Makefile's recipe, built out of tree): every
    copy replayed 16 bytes at a time through fanout_pay_piece between exact-size
    heap buffers, against the reference's writes restated byte by byte; a
    program of its own under AddressSanitizer + UBSan, nothing preloaded."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_pay_check: fanout_pay_check\.cpp .*fanout_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_pay_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_pay_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_pay_check: \d+ cases, \d+ copies replayed, [1-9]\d* patched, [1-9]\d* half patches, "
                     r"0 failures", r.stdout)


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
    """As much of a device tensor as the fan-out methods look at."""

    def __init__(self, ptr, nbytes, item=1):
        self.ptr, self.nbytes, self.item = ptr, nbytes, item

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.nbytes // self.item

    def element_size(self):
        return self.item


def test_the_ast_methods_make_the_calls_they_made(monkeypatch):
    """fanout_host_ast / fanout_device_ast reach srtp_fanout_*_ast (or _rw with
    no stamp) with the arguments they always passed; the _pay methods with
    pay=None are those calls, and with records reach srtp_fanout_*_pay with the
    records behind stamp.  Too few records are a ValueError before any call."""
    from libjitsi_amd import SRTPEngine
    lib = Recorder()
    monkeypatch.setattr(N, "lib", lambda: lib)
    eng = SRTPEngine.__new__(SRTPEngine)
    eng.h = 0x1234
    n, m = 3, 2
    src_seg, seg = np.zeros(64, np.uint8), np.zeros(192, np.uint8)
    a32 = lambda k: np.zeros(k, np.uint32)
    host = (7, src_seg, a32(m), a32(m), a32(m), np.zeros(n, np.int32), seg, a32(n), a32(n))
    rw, ast = np.zeros(n, N.FANOUT_REWRITE_DTYPE), np.zeros(n, N.FANOUT_AST_DTYPE)
    pay = np.zeros(n, N.FANOUT_PAYLOAD_DTYPE)

    def last():
        name, args = lib.calls[-1]
        return name, len(args), args

    eng.fanout_host_ast(*host, rewrite=rw, stamp=ast)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_host_ast", 21)
    assert args[0] == 0x1234 and args[1] == src_seg.ctypes.data and args[2] == 64 and args[7] == m
    assert args[9:13] == (None, 7, seg.ctypes.data, 192) and args[16] is None and args[17] is not None
    assert args[18] is not None and args[20] == n
    eng.fanout_host_ast(*host, rewrite=rw)
    assert last()[:2] == ("srtp_fanout_host_rw", 20)
    eng.fanout_host_pay(*host, rewrite=rw, stamp=ast)  # pay=None: the _ast call, exactly
    assert last()[:2] == ("srtp_fanout_host_ast", 21)
    eng.fanout_host_pay(*host)
    assert last()[:2] == ("srtp_fanout_host_rw", 20) and last()[2][17] is None
    eng.fanout_host_pay(*host, pay=pay)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_host_pay", 22)
    assert args[17] is None and args[18] is None and args[19] is not None and args[21] == n
    eng.fanout_host_pay(*host, rewrite=rw, stamp=ast, pay=pay)
    assert all(x is not None for x in last()[2][17:20])
    calls = len(lib.calls)
    with pytest.raises(ValueError):
        eng.fanout_host_pay(*host, pay=pay[:2])
    assert len(lib.calls) == calls

    t = lambda ptr, nbytes, item=4: Tensor(ptr, nbytes, item)
    dev = (7, t(0x1000, 64, 1), t(0x2000, 4 * m), t(0x3000, 4 * m), t(0x4000, 4 * m), t(0x5000, 4 * n),
           t(0x6000, 192, 1), t(0x7000, 4 * n), t(0x8000, 4 * n), t(0x9000, 4 * n), t(0xA000, 4 * n))
    d_rw, d_ast, d_pay = t(0xB000, 16 * n, 1), t(0xC000, 8 * n, 1), t(0xD000, 8 * n, 1)
    eng.fanout_device_ast(*dev, d_rw, d_ast)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_device_ast", 20)
    assert args[:6] == (0x1234, 0x1000, 0x2000, 0x3000, 0x4000, None) and args[6] == m
    assert args[7:10] == (0x5000, None, 7) and args[10:14] == (0x6000, 0x7000, 0x8000, 0x9000)
    assert args[14:] == (None, 0xB000, 0xC000, 0xA000, n, None)
    eng.fanout_device_ast(*dev, None, d_ast)
    assert last()[0] == "srtp_fanout_device_ast" and last()[2][15:17] == (None, 0xC000)
    eng.fanout_device_pay(*dev, d_rw, d_ast, d_pay)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_device_pay", 21)
    assert args[:15] == lib.calls[-3][1][:15] and args[15:] == (0xB000, 0xC000, 0xD000, 0xA000, n, None)
    eng.fanout_device_pay(*dev, None, None, None)
    assert last()[2][15:18] == (None, None, None)
    calls = len(lib.calls)
    for bad in ((t(0xB000, 16 * n - 1, 1), d_ast, d_pay), (d_rw, t(0xC000, 8 * n - 1, 1), d_pay),
                (d_rw, d_ast, t(0xD000, 8 * n - 1, 1))):
        with pytest.raises(ValueError):
            eng.fanout_device_pay(*dev, *bad)
    assert len(lib.calls) == calls
