"""Fan-out that strips or adds RED, as seen without a GPU: the entry points and
the 4-byte record agree between the header, _native.py and the built library; a
NULL engine is refused before any device is touched; srtp_fanout_red_job
(red_job.h's red_wanted and red_rule, the text k_fanout_red compiles) agrees
with red_ref -- the reference's two transform methods restated from the Java
source -- over the grid tools/fanout_red_check runs; that program builds and
runs clean under AddressSanitizer + UBSan; the Python methods make the calls
they should; and every grid the GPU tests run holds, by red_ref alone, each
result code, so that a kernel that answers 0 everywhere cannot pass them."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import red_grids as RG
import red_ref as R
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device_red", "srtp_fanout_host_red", "srtp_fanout_red_job", "srtp_engine_fanout_red_stats")
FIELDS = ["mode", "red_pt", "reserved"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct \{ uint8_t mode, red_pt, reserved\[2\]; \} srtp_fanout_red;", text)
    assert [n for n, _ in N.FanoutRed._fields_] == FIELDS
    assert C.sizeof(N.FanoutRed) == 4 and [getattr(N.FanoutRed, n).offset for n in FIELDS] == [0, 1, 2]
    dt = N.FANOUT_RED_DTYPE
    assert dt.itemsize == 4 and list(dt.names) == FIELDS and [dt.fields[n][1] for n in FIELDS] == [0, 1, 2]
    a = np.zeros(1, dt)
    a["mode"], a["red_pt"], a["reserved"] = 2, 96, (7, 9)
    assert a.tobytes() == bytes([2, 96, 7, 9])
    r = N.FanoutRed.from_buffer_copy(a.tobytes())
    assert (r.mode, r.red_pt, list(r.reserved)) == (2, 96, [7, 9])
    for name, value in (("SRTP_RED_OFF", N.RED_OFF), ("SRTP_RED_STRIP", N.RED_STRIP), ("SRTP_RED_WRAP", N.RED_WRAP),
                        ("SRTP_RED_UNTOUCHED", N.RED_UNTOUCHED), ("SRTP_RED_STRIPPED", N.RED_STRIPPED),
                        ("SRTP_RED_WRAPPED", N.RED_WRAPPED)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert re.search(r"#define SRTP_RED_DROPPED \(-1\)", header) and N.RED_DROPPED == -1
    assert (R.OFF, R.STRIP, R.WRAP) == (N.RED_OFF, N.RED_STRIP, N.RED_WRAP)
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
        if name in ENTRY[:2]:  # red and red_out follow pay
            assert args[args.index("pay") + 1:][:3] == ["red", "red_out", "status"]
    # the plan and the stats; no existing struct grew
    assert [n for n, _ in N.FanoutRedPlan._fields_] == ["result", "h", "len_out", "shift"]
    assert C.sizeof(N.FanoutRedPlan) == 16 and C.sizeof(N.FanoutRedStats) == 32
    assert C.sizeof(N.FanoutStats) == 40 and C.sizeof(N.FanoutPayload) == 8 and C.sizeof(N.Stats) == C.sizeof(N.Stats)
    assert "red_job.h" in N.KERNEL_SOURCES


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    red = (N.FanoutRed * 4)()
    out = (C.c_int8 * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device_red(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                    None, None, None, None, p(red), p(out), p(i), n, None) == -1
    assert L.srtp_fanout_host_red(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                                  p(w), None, None, None, None, p(red), p(out), p(i), n) == -1
    assert L.srtp_engine_fanout_red_stats(None, C.byref(N.FanoutRedStats())) == -1
    plan = N.FanoutRedPlan(7, 7, 7, 7)
    assert L.srtp_fanout_red_job(p(buf), 0, 1, 64, 64, 0, 64, 0, None, C.byref(plan)) == -1
    assert L.srtp_fanout_red_job(p(buf), 0, 1, 64, 64, 0, 64, 0, red, None) == -1
    red[0].mode, red[0].red_pt = 1, 96
    assert L.srtp_fanout_red_job(None, 0, 1, 64, 64, 0, 64, 0, red, C.byref(plan)) == -1  # bytes would be read
    assert (plan.result, plan.h, plan.len_out, plan.shift) == (7, 7, 7, 7)
    red[0].mode = 0
    assert L.srtp_fanout_red_job(None, 0, 1, 64, 64, 0, 64, 0, red, C.byref(plan)) == 0  # off: none is
    assert (plan.result, plan.h, plan.len_out, plan.shift) == (0, 0, 64, 0)


def job(pkt, rec, src_len=None, src_cap=None, dst_cap=None, flags=0, status=0, reserved=(0, 0)):
    L = N.lib()
    r = N.FanoutRed(rec[0], rec[1], (C.c_uint8 * 2)(*reserved))
    plan = N.FanoutRedPlan()
    c = len(pkt)
    buf = (C.c_uint8 * max(c, 1)).from_buffer_copy(bytes(pkt) or b"\0")
    assert L.srtp_fanout_red_job(C.cast(buf, C.c_void_p), 0, 1, c if src_len is None else src_len,
                                 c if src_cap is None else src_cap, status, c + 1 if dst_cap is None else dst_cap,
                                 flags, C.byref(r), C.byref(plan)) == 0
    return plan.result, plan.h, plan.len_out, plan.shift


def sweep():
    """tools/fanout_red_check's grid: c, CC, X, both extension-length bytes, the byte at h (a sample of its
    256 values here; the program takes every one), both modes."""
    lens = (0, 1, 2, 0x7F, 0x80, 0xFF)
    for c in range(12, 97):
        for cc in range(3):
            yield c, cc, None, None
            for l0 in lens:
                for l1 in lens:
                    yield c, cc, l0, l1
    for c in range(12, 41):  # a header's end at 0, 4 and 8
        for cc in range(3):
            for k in (2, 3, 4):
                yield c, cc, 0xFF, 256 - (k + cc)


def test_red_job_agrees_with_the_reference():
    seen = {0: 0, 1: 0, 2: 0, -1: 0}
    cases = 0
    for c, cc, l0, l1 in sweep():
        ext = None if l0 is None else b""
        base = bytearray(RG.packet(0x1234, 9, c, cc, ext, marker=1, at_h=None, ext_len=None if l0 is None else bytes([l0, l1])))
        pkt = R.Pkt(bytes(base))
        try:
            h = pkt.header_length()
        except R.JavaThrow:
            h = -1
        values = (0, 0x45, 0x7F, 0x80, 0xE4) if 0 < h < c else (None,)  # h == 0: the byte there is b0
        for v in values:
            if v is not None:
                base[h] = v
            for mode in (R.STRIP, R.WRAP):
                for pt in ((96, 97) if v in (None, 0x45) else (96,)):
                    want, new = R.apply(bytes(base), (mode, pt))
                    got = job(base, (mode, pt))
                    assert got[0] == want, (c, cc, l0, l1, v, mode, pt, got)
                    if want > 0:
                        assert got[2] == len(new) == c + got[3] and got[3] == (-1 if want == 1 else 1)
                        assert got[1] == R.Pkt(bytes(base)).header_length()
                    else:
                        assert got[1:] == (0, 0 if want < 0 else c, 0)
                    seen[want] += 1
                    cases += 1
    assert cases > 40000 and all(v > 1000 for v in seen.values()), seen
    # when the step is not asked for: result 0 and fanout_job's length
    pkt = RG.packet(1, 2, 60)
    assert job(pkt, (R.STRIP, 96)) == (1, 12, 59, -1)
    assert job(pkt, (R.STRIP, 96), dst_cap=59) == (0, 0, 60, 0)      # truncated by the destination
    assert job(pkt, (R.STRIP, 96), src_cap=59) == (0, 0, 60, 0)      # ... by the source's region
    assert job(pkt, (R.STRIP, 96), flags=N.PKT_FLAG_SKIP) == (0, 0, 0, 0)
    assert job(pkt, (R.STRIP, 96), status=3) == (0, 0, 0, 0)
    assert job(pkt, (3, 96)) == (0, 0, 60, 0) and job(pkt, (R.STRIP, 128)) == (0, 0, 60, 0)
    assert job(pkt, (R.STRIP, 96), reserved=(0, 1)) == (0, 0, 60, 0)
    assert job(pkt[:11], (R.WRAP, 96)) == (0, 0, 11, 0)
    assert job(pkt, (R.WRAP, 96), dst_cap=60) == (2, 12, 61, 1)      # does not fit: still wrapped, len 61


def test_red_ref_by_hand():
    """The restatement against packets worked out by hand."""
    p = RG.packet(0xAABBCCDD, 5, 20, at_h=0x64)
    assert R.apply(p, (R.STRIP, 96)) == (1, p[:1] + b"\x64" + p[2:12] + p[13:])
    assert R.apply(p, (R.WRAP, 101)) == (2, p[:1] + b"\x65" + p[2:12] + b"\x60" + p[12:])
    m = p[:1] + b"\xE0" + p[2:]  # the marker stays
    assert R.apply(m, (R.STRIP, 96))[1][1] == 0xE4 and R.apply(m, (R.WRAP, 101))[1][1] == 0xE5
    assert R.apply(p[:12] + b"\xE4" + p[13:], (R.STRIP, 96)) == (-1, None)  # F set
    assert R.apply(p, (R.OFF, 96)) == (0, p) and R.apply(p, (R.STRIP, 97)) == (0, p)
    x = RG.packet(1, 2, 40, 0, RG.EL, ext_len=b"\xFF\xFC")  # h == 0
    got = R.apply(x, (R.WRAP, 101))
    assert got == (2, bytes([x[1] & 0x7F, 0x80 | 101]) + x[1:])


def test_fanout_red_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_red_check (the Makefile's recipe, built out of tree): a
    program of its own under AddressSanitizer + UBSan, nothing preloaded."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_red_check: fanout_red_check\.cpp .*red_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_red_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_red_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_red_check: \d+ cases, [1-9]\d* stripped, [1-9]\d* wrapped, [1-9]\d* dropped, "
                     r"[1-9]\d* untouched, [1-9]\d* pieces, 0 failures", r.stdout)


@pytest.mark.parametrize("room", [10, 16])
def test_every_gpu_grid_holds_every_code(room):
    """By red_ref alone: each grid of tests/test_fanout_red.py has entries that
    are untouched, stripped, wrapped and dropped."""
    for make in (RG.boundaries, RG.pairs, RG.answers, RG.together):
        codes = RG.codes(make(room), room)
        assert set(codes) == {0, 1, 2, -1}, (make.__name__, sorted(set(codes)))
        assert min(codes.count(k) for k in (0, 1, 2, -1)) >= 1
    a = RG.answers(room)  # the codes worked out by hand
    assert len(a) == 30 and RG.codes(a, room) == [e["want"] for e in a]
    for g in (a, RG.boundaries(room)):  # the entries the chain refuses as malformed stand last
        bad = [RG.malformed(e, room) for e in g]
        assert any(bad) and bad == sorted(bad)
    assert RG.codes(RG.together(room), room) == [1, 2, -1, 0]
    g = RG.pairs(room)
    assert len(g) == 73 and RG.codes(g, room).count(-1) == 12
    # a wrap that fits exactly and one that does not are both wrapped by the rule
    b = RG.boundaries(room)
    tight = [j for j, e in enumerate(b) if e["cap"] is not None and e["cap"] <= len(e["pkt"]) + 1]
    assert len(tight) == 8 and all(RG.codes(b, room)[j] == 2 for j in tight)


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
    import libjitsi_amd as J
    from libjitsi_amd import SRTPEngine, fan_out_red
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device_red) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                                 "seg", "off", "length", "cap", "status", "rewrite", "stamp", "pay",
                                                 "red", "red_out", "src_status", "flags", "m", "n", "stream"]
    assert sig(SRTPEngine.fanout_host_red) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                               "seg", "off", "cap", "src_status", "flags", "rewrite", "stamp", "pay",
                                               "red"]
    assert sig(fan_out_red) == ["pkts", "transformers", "rewriters", "stampers", "payers", "reds", "exclusion"]
    assert (J.RED_OFF, J.RED_STRIP, J.RED_WRAP) == (0, 1, 2)
    for f in (fan_out_red, SRTPEngine.fanout_device_red, SRTPEngine.fanout_host_red):
        assert "REDFilterTransformEngine.java:95-145" in f.__doc__ and "REDTransformEngine.java:151-182" in f.__doc__
    assert fan_out_red([], [], [], [], [], []) == ([], [])
    for bad in (([None], [], [], []), ([], [None], [], []), ([], [], [None], []), ([], [], [], [None])):
        with pytest.raises(ValueError):
            fan_out_red([], [], *bad)

    lib = Recorder()
    monkeypatch.setattr(N, "lib", lambda: lib)
    eng = SRTPEngine.__new__(SRTPEngine)
    eng.h = 0x1234
    n, m = 3, 2
    src_seg, seg = np.zeros(64, np.uint8), np.zeros(192, np.uint8)
    a32 = lambda k: np.zeros(k, np.uint32)
    host = (7, src_seg, a32(m), a32(m), a32(m), np.zeros(n, np.int32), seg, a32(n), a32(n))
    pay, red = np.zeros(n, N.FANOUT_PAYLOAD_DTYPE), np.zeros(n, N.FANOUT_RED_DTYPE)
    last = lambda: (lib.calls[-1][0], len(lib.calls[-1][1]), lib.calls[-1][1])
    ln, st, ro = eng.fanout_host_red(*host)  # red=None: the _pay call, which without records is the _rw call
    assert last()[:2] == ("srtp_fanout_host_rw", 20) and ro.dtype == np.int8 and ro.tolist() == [0] * n
    eng.fanout_host_red(*host, pay=pay)
    assert last()[:2] == ("srtp_fanout_host_pay", 22)
    ln, st, ro = eng.fanout_host_red(*host, red=red)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_host_red", 24)
    assert args[0] == 0x1234 and args[1] == src_seg.ctypes.data and args[2] == 64 and args[7] == m
    assert args[17:20] == (None, None, None) and args[20] is not None and args[21] == ro.ctypes.data and args[23] == n
    eng.fanout_host_red(*host, pay=pay, red=red)
    assert last()[2][19] is not None
    calls = len(lib.calls)
    with pytest.raises(ValueError):
        eng.fanout_host_red(*host, red=red[:2])
    assert len(lib.calls) == calls

    t = lambda ptr, nbytes, item=4: Tensor(ptr, nbytes, item)
    dev = (7, t(0x1000, 64, 1), t(0x2000, 4 * m), t(0x3000, 4 * m), t(0x4000, 4 * m), t(0x5000, 4 * n),
           t(0x6000, 192, 1), t(0x7000, 4 * n), t(0x8000, 4 * n), t(0x9000, 4 * n), t(0xA000, 4 * n))
    d_pay, d_red, d_out = t(0xD000, 8 * n, 1), t(0xE000, 4 * n, 1), t(0xF000, n, 1)
    eng.fanout_device_red(*dev, None, None, d_pay, d_red, d_out)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_device_red", 23)
    assert args[:6] == (0x1234, 0x1000, 0x2000, 0x3000, 0x4000, None) and args[6] == m
    assert args[7:10] == (0x5000, None, 7) and args[10:14] == (0x6000, 0x7000, 0x8000, 0x9000)
    assert args[14:] == (None, None, None, 0xD000, 0xE000, 0xF000, 0xA000, n, None)
    eng.fanout_device_red(*dev, None, None, None, None, None)
    assert last()[2][15:20] == (None,) * 5
    calls = len(lib.calls)
    for bad in ((d_pay, t(0xE000, 4 * n - 1, 1), d_out), (d_pay, d_red, t(0xF000, n - 1, 1)),
                (d_pay, d_red, t(0xF000, 4 * n, 4))):
        with pytest.raises(ValueError):
            eng.fanout_device_red(*dev, None, None, *bad)
    assert len(lib.calls) == calls


def test_fan_out_red_makes_one_host_call(monkeypatch):
    """fan_out_red lays the records out per destination entry (packet-major, a
    transformer's mode on its stride) and reaches fanout_host_red once; without
    any mode it still goes through it, with red None."""
    import libjitsi_amd.srtp as S
    from libjitsi_amd import RawPacket, fan_out_red
    seen = []

    class Eng(S.SRTPEngine):
        trailer_room = 10

        def __init__(self):
            pass

        def fanout_host_red(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap, src_status=None,
                            flags=None, rewrite=None, stamp=None, pay=None, red=None):
            seen.append(dict(tid=tid, cap=np.array(cap), rewrite=rewrite, stamp=stamp, pay=pay, red=red,
                             src_len=np.array(src_len)))
            n = len(off)
            ro = np.zeros(n, np.int8) if red is None else red["mode"].astype(np.int8)
            return np.zeros(n, np.uint32), np.full(n, N.STATUS_SKIPPED, np.int32), ro

    eng = Eng()

    class T:
        packetPredicate = None

        def __init__(self, tid):
            self.engine, self.tid = eng, tid

    ts = [T(3), T(4), T(5)]
    pk = [RawPacket(RG.packet(10 + i, i, 40 + i), 0, 40 + i) for i in range(2)]
    out, codes = fan_out_red(pk, ts, [None] * 3, [None] * 3, [None, lambda p: {"osn": 0xBEEF}, None],
                             [(S.RED_STRIP, 96), None, (S.RED_WRAP, 101)])
    assert len(seen) == 1 and out == [[None, None]] * 3 and codes == [[1, 1], [0, 0], [2, 2]]
    c = seen[0]
    assert c["red"]["mode"].tolist() == [1, 0, 2, 1, 0, 2] and c["red"]["red_pt"].tolist() == [96, 0, 101, 96, 0, 101]
    assert c["tid"].tolist() == [3, 4, 5, 3, 4, 5] and c["rewrite"] is None and c["stamp"] is None
    assert c["pay"]["at1"].tolist() == [0, 12, 0, 0, 12, 0] and c["pay"]["b1"][1].tolist() == [0xBE, 0xEF]
    assert (c["cap"] - np.repeat(c["src_len"], 3)).tolist() == [10, 10, 11] * 2  # a wrapped copy is one byte longer
    fan_out_red(pk, ts, [None] * 3, [None] * 3, [None] * 3, [None, (S.RED_OFF, 0), None])
    assert len(seen) == 2 and seen[1]["red"] is None and seen[1]["pay"] is None
    with pytest.raises(ValueError):
        fan_out_red(pk, ts, [None] * 3, [None] * 3, [None] * 3, [(3, 96), None, None])
    with pytest.raises(ValueError):
        fan_out_red(pk, ts, [None] * 3, [None] * 3, [None] * 3, [(1, 128), None, None])
    assert len(seen) == 2
