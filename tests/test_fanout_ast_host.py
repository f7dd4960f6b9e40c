"""Fan-out that stamps abs-send-time, as seen without a GPU: the entry points
and the 8-byte record agree between the header, _native.py and the built
library; a NULL engine is refused before any device is touched;
srtp_fanout_ast_job (fanout_job.h's fanout_ast_find, the text k_fanout_ast
compiles) agrees with abs_send_time_ref.find -- AbsSendTimeEngine's walk restated
with Java's signed bytes -- over the shapes tests/test_fanout_ast.py runs on the
device; tools/fanout_ast_check builds and runs clean under AddressSanitizer +
UBSan; fan_out_ast of nothing is nothing."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import abs_send_time_ref as A
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device_ast", "srtp_fanout_host_ast", "srtp_fanout_ast_job")
SKIP = N.PKT_FLAG_SKIP
FIELDS = ["value", "id", "on", "reserved"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_fanout_abs_send_time;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint32_t value; uint8_t id, on; uint16_t reserved;"
    assert [n for n, _ in N.FanoutAbsSendTime._fields_] == FIELDS
    assert C.sizeof(N.FanoutAbsSendTime) == 8
    assert [getattr(N.FanoutAbsSendTime, n).offset for n in FIELDS] == [0, 4, 5, 6]
    dt = N.FANOUT_AST_DTYPE
    assert dt.itemsize == 8 and list(dt.names) == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 4, 5, 6]
    # stamp follows rewrite in both entries
    for name in ENTRY[:2]:
        proto = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        args = [a.strip().split("*")[-1].split()[-1] for a in proto.split(",")]
        assert args[args.index("flags") + 1] == "rewrite" and args[args.index("rewrite") + 1] == "stamp"
        assert args[args.index("stamp") + 1] == "status"
    assert int(re.search(r"#define SRTP_MI355X_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION
    # no existing struct grew
    assert C.sizeof(N.FanoutStats) == 40 and C.sizeof(N.FanoutRewrite) == 16


def test_record_dtype_round_trips():
    """A numpy record and the ctypes struct are the same 8 bytes."""
    a = np.zeros(1, N.FANOUT_AST_DTYPE)
    a["value"], a["id"], a["on"], a["reserved"] = 0x00C1D2E3, 3, 1, 0xBEEF
    assert a.tobytes() == bytes([0xE3, 0xD2, 0xC1, 0x00, 3, 1, 0xEF, 0xBE])
    r = N.FanoutAbsSendTime.from_buffer_copy(a.tobytes())
    assert (r.value, r.id, r.on, r.reserved) == (0x00C1D2E3, 3, 1, 0xBEEF)


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    rw = (N.FanoutRewrite * 4)()
    ast = (N.FanoutAbsSendTime * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device_ast(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                    None, p(rw), p(ast), p(i), n, None) == -1
    assert L.srtp_fanout_host_ast(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                                  p(w), None, p(rw), p(ast), p(i), n) == -1
    out = C.c_int32(7)
    assert L.srtp_fanout_ast_job(p(buf), 64, 0, 1, 64, 64, 0, 64, 0, None, C.byref(out)) == -1
    assert L.srtp_fanout_ast_job(p(buf), 64, 0, 1, 64, 64, 0, 64, 0, ast, None) == -1
    assert L.srtp_fanout_ast_job(None, 64, 0, 1, 64, 64, 0, 64, 0, ast, C.byref(out)) == -1
    assert out.value == 7


def test_python_mirrors():
    from libjitsi_amd import SRTPEngine, abs_send_time, fan_out_ast
    import libjitsi_amd.srtp as S
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device_ast) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                                 "seg", "off", "length", "cap", "status", "rewrite", "stamp",
                                                 "src_status", "flags", "m", "n", "stream"]
    assert sig(SRTPEngine.fanout_host_ast) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                               "seg", "off", "cap", "src_status", "flags", "rewrite", "stamp"]
    assert sig(fan_out_ast) == ["pkts", "transformers", "rewriters", "stampers", "exclusion"]
    for f in (S.fan_out_ast, SRTPEngine.fanout_device_ast, SRTPEngine.fanout_host_ast):
        assert "AbsSendTimeEngine.java:86-152" in f.__doc__ and "MediaStreamImpl.java:1018-1035" in f.__doc__
    assert fan_out_ast([], [], [], []) == []
    assert fan_out_ast([None], [], [], []) == []
    with pytest.raises(ValueError):
        fan_out_ast([], [], [], [None])
    with pytest.raises(ValueError):
        fan_out_ast([], [], [None], [])
    # AbsSendTimeEngine.setTimestamp: seconds mod 64 in the top 6 bits, the fraction in 18
    b = 10 ** 9
    assert abs_send_time(0) == 0 and abs_send_time(b) == 1 << 18 and abs_send_time(64 * b) == 0
    assert abs_send_time(b // 2) == 1 << 17 and abs_send_time(63 * b + b - 1) == (63 << 18) | ((b - 1) * (1 << 18) // b)
    assert abs_send_time(12345678901234567) == (((12345678901234567 // b) % 64) << 18) | (901234567 * 2 ** 18 // b)
    assert all(0 <= abs_send_time(ns) < 1 << 24 for ns in (1, 999999999, 2 ** 63 - 1))
    with pytest.raises(ValueError):
        abs_send_time(-1)


# ------------------------------------------------------------------ the sweep
def packets():
    """(packet, a place of interest) over the device test's shapes."""
    body = lambda front, last=True: A.one_byte_ext(
        A.filler(front) + [(3, b"\xA0\xA1\xA2")] + ([(7, b"\x70\x71\x72\x73")] if last else []))
    words_of = A.low_words
    for cc in (0, 1, 15):
        first = 12 + 4 * cc + 4 + 1
        for base in (0, 16, 63 * 16, 127 * 16):
            for res in range(16):
                front = base + res - first
                while front < 0 or front == 1:
                    front += 16
                b = words_of(body(front))
                yield A.rtp_ext(0x1234, 7, b, bytes(range(40)), cc=cc), first + front
        for ln in range(16):
            b = body(ln + 2, bool(ln & 1))
            yield A.rtp_ext(0x1234, 7, b, bytes(20), cc=cc), first + ln + 2
        yield A.rtp_ext(0x1234, 7, body(0, False), b"", cc=cc), first
    b = body(6)
    at = 16 + 6 + 1
    for words in (len(b) // 4, 0, 1, 0x0080, 0x00FF, 0x8000, 0x8001, 0x7F7F, 0xFFFF, 0x7FFF, len(b) // 4 + 1000):
        for profile in (0xBEDE, 0x1000, 0, 0xFFFF):
            yield A.rtp_ext(0x1234, 7, b, bytes(range(30)), words=words, profile=profile), at
    for b0 in (0x80, 0x10, 0x50, 0xD0, 0x00, 0xB0, 0x9F):
        yield A.rtp_ext(0x1234, 7, b, bytes(range(30)), b0=b0), at
    for past in range(6):  # in and just behind the four overshoot bytes
        x = A.one_byte_ext([(5, bytes(6)), 1 + past, (3, b"\xA0\xA1\xA2")], pad_to_word=False)
        yield A.rtp_ext(0x1234, 7, x + b"\x11" * (-len(x) % 4), bytes(range(24)), words=2), 16 + 8 + past + 1
    for pad in range(1, 7):
        yield A.rtp_ext(0x1234, 7, A.one_byte_ext([pad, (3, b"\xA0\xA1\xA2"), (7, b"pq")]), bytes(24)), 16 + pad + 1
    for ln in (0, 1, 3, 15):
        yield A.rtp_ext(0x1234, 7, A.one_byte_ext([(3, bytes(ln + 1)), (3, b"\xA0\xA1\xA2")]), bytes(24)), 16 + ln + 3
    for n in range(12, 25):
        yield A.rtp_ext(0x1234, 7, b"", b"", words=4, b0=0x9F)[:n].ljust(n, b"\x33"), n


RECORDS = ((0x00C1D2E3, 3, 1, 0), (0xFF010203, 3, 1, 0xFFFF), (0x00C1D2E3, 3, 0, 0), (0x00C1D2E3, 16, 1, 0),
           (0x00C1D2E3, 255, 1, 0), (0x00C1D2E3, 0, 1, 0), (0x00C1D2E3, 5, 1, 0), (0x00C1D2E3, 7, 2, 0))


def sweep():
    """(packet, src_idx, m, src_len, src_cap, src_status, dst_cap, flags, record)"""
    for p, around in packets():
        n = len(p)
        for r in RECORDS:
            yield p, 0, 1, n, n, 0, n + 10, 0, r
            for d in range(-4, 7):
                cut = around + d
                if 0 <= cut <= n:
                    yield p, 0, 1, cut, n, 0, n + 10, 0, r
                    yield p, 0, 1, n, n, 0, cut, 0, r
                    yield p, 0, 1, n, cut, 0, n + 10, 0, r
        r = RECORDS[0]
        for fl, idx, m, st in ((SKIP, 0, 1, 0), (SKIP | 4, 0, 1, 0), (0, 0, 1, 2), (0, 1, 1, 0), (0, -1, 3, 0)):
            yield p, idx, m, n, n, st, n + 10, fl, r
        for c in range(14):
            yield p, 0, 1, n, n, 0, c, 0, r
        for L, sc, dc in ((-1, n, n), (n, -1, n), (n, n, -1), (2 ** 31 - 1, n, n)):
            yield p, 0, 1, L, sc, 0, dc, 0, r


def want(p, idx, m, L, sc, st, dc, fl, r):
    """fanout_job's skip rules, then the reference over the c copied bytes."""
    if idx < 0 or idx >= m or st != 0 or fl & SKIP or min(L, sc, dc) < 12:
        return -1
    return A.apply(bytearray(p[:min(L, sc, dc)]), r)


def test_ast_job_agrees_with_the_reference():
    job = N.lib().srtp_fanout_ast_job
    out, rec = C.c_int32(), N.FanoutAbsSendTime()
    cases = stamped = 0
    for p, idx, m, L, sc, st, dc, fl, r in sweep():
        rec.value, rec.id, rec.on, rec.reserved = r
        assert job(p, len(p), idx, m, L, sc, st, dc, fl, C.byref(rec), C.byref(out)) == 0
        w = want(p, idx, m, L, sc, st, dc, fl, r)
        assert out.value == w, (p.hex(), idx, m, L, sc, st, dc, fl, r, out.value, w)
        cases += 1
        stamped += w >= 0
    assert cases > 50000 and stamped > 5000


def test_reference_restates_the_quirks():
    """The restatement against bytes worked out by hand from AbsSendTimeEngine.java:86-130."""
    el = b"\x32\xA0\xA1\xA2"
    p = A.rtp_ext(1, 1, el, b"pay")
    assert A.find(bytearray(p), 3) == 17 and A.find(bytearray(p), 4) == -1 and A.find(bytearray(p), -1) == -1
    assert A.find(bytearray(p[:19]), 3) == -1 and A.find(bytearray(p[:20]), 3) == 17  # p + 3 < buf.length
    assert A.find(bytearray(A.rtp_ext(1, 1, el, b"", words=0x0080)), 3) == -1        # low byte sign-extends
    assert A.find(bytearray(A.rtp_ext(1, 1, el, b"", words=0x8000)), 3) == -1
    assert A.find(bytearray(A.rtp_ext(1, 1, el, b"", words=0, profile=0x1000)), 3) == 17  # 4 * (1 + 0) bytes walked
    assert A.find(bytearray(A.rtp_ext(1, 1, bytes(4), el + b"xx", words=1)), 3) == 21     # the overshoot: payload
    assert A.find(bytearray(A.rtp_ext(1, 1, bytes(8), el + b"xx", words=1)), 3) == -1
    assert A.find(bytearray(A.rtp_ext(1, 1, b"\x00" + el + bytes(3), b"")), 3) == -1      # one padding byte skips two
    assert A.find(bytearray(A.rtp_ext(1, 1, b"\x00\x00" + el + bytes(2), b"")), 3) == 19
    assert A.find(bytearray(A.rtp_ext(1, 1, b"\x00\x00" + el + bytes(2), b"")), 0) == -1  # ID 0 meets padding: len 0
    assert A.find(bytearray(A.rtp_ext(1, 1, b"\x31\x00\x00\x00" + el, b"")), 3) == -1     # the first match decides
    assert A.find(bytearray(A.rtp_ext(1, 1, el, b"", b0=0x50)), 3) == -1 and A.find(bytearray(A.rtp_ext(1, 1, el, b"", b0=0x80)), 3) == -1
    b = bytearray(p)
    assert A.stamp(b, 3, 0xC1D2E3) == 17 and bytes(b) == p[:17] + b"\xC1\xD2\xE3" + p[20:]
    assert A.apply(bytearray(p), (5, 16, 1)) == -1 and A.apply(bytearray(p), (5, 3, 0)) == -1


def test_fanout_ast_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_ast_check (the Makefile's recipe, built out of tree): every
    copy replayed 16 bytes at a time through fanout_ast_piece between
    exact-size heap buffers, against AbsSendTimeEngine restated with int8_t
    bytes; a program of its own under AddressSanitizer + UBSan."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_ast_check: fanout_ast_check\.cpp .*fanout_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_ast_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_ast_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_ast_check: \d+ cases, \d+ copies replayed, [1-9]\d* stamped, 0 failures", r.stdout)
