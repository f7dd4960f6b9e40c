"""What of the fan-out FEC step (srtp_fanout_device_fec / _host_fec,
k_fanout_fec) can be held without a GPU: the entry points and the record's
layout, the rule (libjitsi_amd/csrc/fec_job.h through srtp_fanout_fec_job)
against FECSender.FECPacket restated (tests/fec_ref.py), fec_ref itself by hand,
the sanitizer check program, the grids the GPU tests run, and the Python
mirrors' arithmetic."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fec_grids as FG
import fec_ref as F
import red_grids as RG
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device_fec", "srtp_fanout_host_fec", "srtp_fanout_fec_job", "srtp_engine_fanout_fec_stats")
FIELDS = ["first", "ssrc", "count", "pt", "red_pt", "mode"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct \{ uint32_t first, ssrc; uint8_t count, pt, red_pt, mode; \} srtp_fanout_fec;", text)
    assert [n for n, _ in N.FanoutFec._fields_] == FIELDS
    offsets = [0, 4, 8, 9, 10, 11]
    assert C.sizeof(N.FanoutFec) == 12 and [getattr(N.FanoutFec, n).offset for n in FIELDS] == offsets
    dt = N.FANOUT_FEC_DTYPE
    assert dt.itemsize == 12 and list(dt.names) == FIELDS and [dt.fields[n][1] for n in FIELDS] == offsets
    a = np.zeros(1, dt)
    a[0] = (0x01020304, 0xA1B2C3D4, 5, 116, 96, 2)
    assert a.tobytes() == bytes([4, 3, 2, 1, 0xD4, 0xC3, 0xB2, 0xA1, 5, 116, 96, 2])
    r = N.FanoutFec.from_buffer_copy(a.tobytes())
    assert (r.first, r.ssrc, r.count, r.pt, r.red_pt, r.mode) == (0x01020304, 0xA1B2C3D4, 5, 116, 96, 2)
    for name, value in (("SRTP_FEC_OFF", N.FEC_OFF), ("SRTP_FEC_PLAIN", N.FEC_PLAIN), ("SRTP_FEC_RED", N.FEC_RED),
                        ("SRTP_FEC_NONE", N.FEC_NONE), ("SRTP_FEC_MADE", N.FEC_MADE)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert re.search(r"#define SRTP_FEC_REFUSED \(-1\)", header) and N.FEC_REFUSED == -1
    assert (FG.PLAIN, FG.RED) == (N.FEC_PLAIN, N.FEC_RED)
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
        if name in ENTRY[:2]:  # the four new arguments follow red_out
            assert args[args.index("red_out") + 1:][:5] == ["fec", "members", "n_members", "fec_out", "status"]
            red = re.search(r"int %s\(([^;]*)\);" % name.replace("_fec", "_red"), text).group(1)
            mine = [d for d, a in zip(decl, args) if a not in ("fec", "members", "n_members", "fec_out")]
            assert mine == [a.strip() for a in red.split(",")]  # the _red call's arguments otherwise
    assert [n for n, _ in N.FanoutFecStats._fields_] == ["calls", "made", "refused", "member_bytes"]
    assert C.sizeof(N.FanoutFecStats) == 32 and C.sizeof(N.FanoutStats) == 40 and C.sizeof(N.FanoutRed) == 4
    assert "fec_job.h" in N.KERNEL_SOURCES


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    fec = (N.FanoutFec * 4)()
    out = (C.c_int8 * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device_fec(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                    None, None, None, None, None, None, p(fec), p(i), 4, p(out), p(i), n, None) == -1
    assert L.srtp_fanout_host_fec(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                                  p(w), None, None, None, None, None, None, p(fec), p(i), 4, p(out), p(i), n) == -1
    assert L.srtp_engine_fanout_fec_stats(None, C.byref(N.FanoutFecStats())) == -1
    ln, code = C.c_int32(7), C.c_int8(7)
    assert L.srtp_fanout_fec_job(None, p(buf), p(w), p(w), p(buf), 64, C.byref(ln), C.byref(code)) == -1
    assert L.srtp_fanout_fec_job(fec, p(buf), p(w), p(w), p(buf), 64, None, C.byref(code)) == -1
    assert (ln.value, code.value) == (7, 7)
    fec[0].mode, fec[0].count = 1, 1
    assert L.srtp_fanout_fec_job(fec, None, p(w), p(w), p(buf), 64, C.byref(ln), C.byref(code)) == -1  # bytes would be read
    fec[0].mode = 0
    assert L.srtp_fanout_fec_job(fec, None, None, None, None, 0, C.byref(ln), C.byref(code)) == 0  # off: none is
    assert (ln.value, code.value) == (0, 0)


def job(members, ssrc, pt, red_pt=None, out_cap=None, over=None):
    """srtp_fanout_fec_job over the members: (code, len_out, bytes)."""
    rec = N.FanoutFec(3, ssrc, len(members), pt, red_pt if red_pt is not None else 0, 1 if red_pt is None else 2)
    for k, v in (over or {}).items():
        setattr(rec, k, v)
    blob = b"".join(members) or b"\0"
    at = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint32) if members else np.zeros(1, np.uint32)
    lens = np.array([len(m) for m in members] or [0], np.uint32)
    cap = max((len(m) for m in members), default=12) + 40 if out_cap is None else out_cap
    out = (C.c_uint8 * max(cap, 1))(*([0xEE] * max(cap, 1)))
    ln, code = C.c_int32(), C.c_int8()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    assert N.lib().srtp_fanout_fec_job(C.byref(rec), C.cast(buf, C.c_void_p), at.ctypes.data, lens.ctypes.data,
                                       C.cast(out, C.c_void_p), cap, C.byref(ln), C.byref(code)) == 0
    return code.value, ln.value, bytes(out)


def test_fec_job_agrees_with_the_reference():
    """Counts 1..16, both modes, member lengths around every piece boundary, alone and mixed, against fec_ref;
    a destination shorter than the packet gets its first bytes and nothing behind them."""
    rng = np.random.default_rng(5109)
    single = (12, 13, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1008, 1010, 1012, 1200, 2032, 2034, 2036)
    cases = 0
    for red_pt in (None, 101):
        for count in range(1, 17):
            for trial in range(6):
                longest = single[(count * 7 + trial * 5) % len(single)]
                lens = [int(rng.integers(12, longest + 1)) for _ in range(count)]
                lens[(trial * count // 6) % count] = longest
                members = []
                for i, c in enumerate(lens):
                    b = bytearray(rng.integers(0, 256, c, np.uint8).tobytes())
                    b[0] = 0x80 | (b[0] & 0x3F)
                    members.append(bytes(b))
                want = F.make(members, 0xCAFE0000 + count, 100 + trial, red_pt)
                code, ln, out = job(members, 0xCAFE0000 + count, 100 + trial, red_pt)
                assert (code, ln) == (1, len(want)) and out[:ln] == want, (count, lens, red_pt)
                assert set(out[ln:]) <= {0xEE}
                short = len(want) - 1 - trial
                code, ln, out = job(members, 0xCAFE0000 + count, 100 + trial, red_pt, out_cap=short)
                assert (code, ln) == (1, len(want)) and out[:short] == want[:short]
                cases += 1
    assert cases == 192
    good = [RG.packet(7, i, 40 + i) for i in range(3)]
    assert job(good, 1, 2)[0] == 1
    for over in (dict(count=0), dict(count=17), dict(pt=128), dict(mode=3), dict(mode=2, red_pt=128)):
        assert job(good * 6, 1, 2, over=over)[:2] == (-1, 0), over
    assert job(good, 1, 2, over=dict(red_pt=255))[0] == 1  # red_pt is not looked at when plain
    assert job([good[0], good[1][:11]], 1, 2)[:2] == (-1, 0)                  # a member shorter than 12
    assert job([good[0], RG.packet(7, 9, 40, version=1)], 1, 2)[:2] == (-1, 0)  # not version 2


def test_fec_ref_by_hand():
    """One three-packet group written out: the header fields and the XOR worked out by hand."""
    a = bytes.fromhex("80e4 0010 00000100 11111111") + bytes([0x01, 0x02, 0x03, 0x04])
    b = bytes.fromhex("90e4 0011 00000200 11111111") + bytes([0x10, 0x20])
    c = bytes.fromhex("80e4 0012 00000400 11111111") + bytes([0xFF, 0x00, 0xFF, 0x00, 0xFF, 0x07])
    got = F.make([a, b, c], 0x22222222, 0x74)
    want = (bytes.fromhex("80 74 0013 00000400 22222222")        # PT, last seq + 1, last timestamp, ssrc
            + bytes.fromhex("90 e4 0010 00000700")               # byte 12: 80^90^80 (E set), e4^e4^e4, SN base, TS xor
            + bytes.fromhex("0000")                              # length recovery 4 ^ 2 ^ 6
            + bytes.fromhex("0006 e000")                         # protection length, mask of three
            + bytes([0x01 ^ 0x10 ^ 0xFF, 0x02 ^ 0x20, 0x03 ^ 0xFF, 0x04, 0xFF, 0x07]))
    assert got == want and len(got) == 26 + 6
    wrapped = F.make([a, b, c], 0x22222222, 0x74, 0x60)
    assert wrapped == want[:1] + b"\x60" + want[2:12] + b"\x74" + want[12:]
    assert F.make([a], 5, 0x74)[12:26] == a[:2] + a[2:4] + a[4:8] + bytes.fromhex("0004 0004 8000")
    seqs = [RG.packet(9, (0xFFFF + i) & 0xFFFF, 20) for i in range(16)]
    assert F.make(seqs[:1], 5, 1)[2:4] == b"\x00\x00" and F.make(seqs, 5, 1)[24:26] == b"\xFF\xFF"
    for lost in range(3):  # RFC 5109 9.2 gives each packet back
        others = [p for i, p in enumerate((a, b, c)) if i != lost]
        rec = F.recover(got, others)
        full = (a, b, c)[lost]
        assert rec[:8] == full[:8] and rec[12:] == full[12:] and rec[8:12] == got[8:12]


def test_fanout_fec_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_fec_check (the Makefile's recipe, built out of tree): a
    program of its own under AddressSanitizer + UBSan, nothing preloaded."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_fec_check: fanout_fec_check\.cpp .*fec_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_fec_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_fec_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_fec_check: [1-9]\d* packets, [1-9]\d* pieces, [1-9]\d* refusal checks, 0 failures", r.stdout)


COUNTS = {  # grid: (entries, made, refused) -- what the GPU tests assert
    "boundaries": (160, 96, 1), "with_records": (15, 4, 1), "shared": (18, 6, 1), "many": (393, 130, 1),
    "refusals_host": (20, 3, 6), "refusals_device": (33, 5, 16), "all_refused": (8, 0, 5),
}


@pytest.mark.parametrize("room", [10, 16])
def test_every_gpu_grid_holds_every_code(room):
    """By fec_ref alone: each grid of tests/test_fanout_fec.py has entries with code 0, made and refused (the
    grid that is all refused has none made), in the counts the GPU tests assert."""
    grids = {"boundaries": FG.boundaries(room), "with_records": FG.with_records(room), "shared": FG.shared(room),
             "many": FG.many(130), "refusals_host": FG.refusals(room, False), "refusals_device": FG.refusals(room, True),
             "all_refused": FG.all_refused(room)}
    for name, g in grids.items():
        codes, packets, member_bytes = FG.expect(g, room)
        assert (len(g), codes.count(1), codes.count(-1)) == COUNTS[name], name
        assert set(codes) == ({0, 1, -1} if name != "all_refused" else {0, -1}), name
        assert len(packets) == codes.count(1) and member_bytes == sum(
            sum(len(FG.final(g[mi], room)[0]) - 4 for mi in g[j]["fec"]["members"]) for j in packets)
        rec, members = FG.arrays(g)
        assert len(rec) == len(g) and (rec["mode"] != 0).sum() == sum(
            1 for e in g if e["fec"] is not None and e["fec"]["mode"] != 0)
        for j, e in enumerate(g):
            if e["fec"] is not None and not FG.field_causes(g, j) and e["fec"]["mode"]:
                first, count = int(rec["first"][j]), int(rec["count"][j])
                assert members[first:first + count].tolist() == e["fec"]["members"]
    # the host route's grid has no entry the host route answers with SRTP_EINVAL; the device route's has one of each
    g = grids["refusals_host"]
    assert not any(FG.field_causes(g, j) for j, e in enumerate(g) if e["fec"] is not None)
    g = grids["refusals_device"]
    causes = [c for j, e in enumerate(g) if e["fec"] is not None and e["fec"]["mode"] for c in FG.field_causes(g, j)]
    assert set(causes) == {"mode", "count", "first + count", "pt", "src_idx", "member index", "member record"}
    # plain and wrapped differ by the one byte; a packet one byte short of its region is still made
    b = grids["boundaries"]
    codes, packets, _ = FG.expect(b, room)
    tight = [j for j, e in enumerate(b) if e["fec"] is not None and e["cap"] is not None]
    assert len(tight) == 24 and all(codes[j] == 1 for j in tight)
    assert sorted({len(packets[j]) - e["cap"] for j, e in ((j, b[j]) for j in tight)}) == [-room, 0, 1]
    # two peers with different rewrites get different packets over the same sources
    r = grids["with_records"]
    _, packets, _ = FG.expect(r, room)
    plain = [packets[j] for j, e in enumerate(r) if j in packets and e["fec"]["mode"] == FG.PLAIN]
    assert len(plain) == 2 and plain[0] != plain[1] and len(plain[0]) == len(plain[1])


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
    from libjitsi_amd import FecSender, SRTPEngine, fan_out_fec
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device_fec) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                                 "seg", "off", "length", "cap", "status", "rewrite", "stamp", "pay",
                                                 "red", "red_out", "fec", "members", "fec_out", "src_status", "flags",
                                                 "m", "n", "n_members", "stream"]
    assert sig(SRTPEngine.fanout_host_fec) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                               "seg", "off", "cap", "src_status", "flags", "rewrite", "stamp", "pay",
                                               "red", "fec", "members"]
    assert sig(fan_out_fec) == ["pkts", "transformers", "rewriters", "stampers", "payers", "reds", "fecs", "exclusion"]
    assert sig(FecSender.__init__) == ["self", "ssrc", "rate", "pt", "red_pt"]
    for f in (fan_out_fec, SRTPEngine.fanout_device_fec):
        assert "FECSender" in f.__doc__ and ":319-412" in f.__doc__
    assert "``fec`` key" in fan_out_fec.__doc__ and "makes none" in fan_out_fec.__doc__  # the payers' key keeps its meaning
    assert fan_out_fec([], [], [], [], [], [], []) == ([], [], [])
    for bad in (0, 17):
        with pytest.raises(ValueError):
            FecSender(1, bad, 116)
    with pytest.raises(ValueError):
        FecSender(1, 4, 128)
    with pytest.raises(ValueError):
        FecSender(1, 4, 116, 128)
    s = FecSender(0x1_0000_0001, 4, 116)
    assert (s.ssrc, s.rate, s.pt, s.red_pt, s.counter, s.nb_fec) == (1, 4, 116, None, 0, 0)

    lib = Recorder()
    monkeypatch.setattr(N, "lib", lambda: lib)
    eng = SRTPEngine.__new__(SRTPEngine)
    eng.h = 0x1234
    n, m = 3, 2
    src_seg, seg = np.zeros(64, np.uint8), np.zeros(192, np.uint8)
    a32 = lambda k: np.zeros(k, np.uint32)
    host = (7, src_seg, a32(m), a32(m), a32(m), np.zeros(n, np.int32), seg, a32(n), a32(n))
    red, fec = np.zeros(n, N.FANOUT_RED_DTYPE), np.zeros(n, N.FANOUT_FEC_DTYPE)
    members = np.array([0, 1], np.int32)
    last = lambda: (lib.calls[-1][0], len(lib.calls[-1][1]), lib.calls[-1][1])
    ln, st, ro, fo = eng.fanout_host_fec(*host, red=red)  # fec=None: the _red call
    assert last()[:2] == ("srtp_fanout_host_red", 24) and fo.dtype == np.int8 and fo.tolist() == [0] * n
    ln, st, ro, fo = eng.fanout_host_fec(*host, fec=fec, members=members)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_host_fec", 28)
    assert args[0] == 0x1234 and args[1] == src_seg.ctypes.data and args[2] == 64 and args[7] == m
    assert args[17:21] == (None, None, None, None) and args[21] == ro.ctypes.data and args[22] is not None
    assert args[23] is not None and args[24] == 2 and args[25] == fo.ctypes.data and args[27] == n
    eng.fanout_host_fec(*host, fec=fec)
    assert last()[2][23:25] == (None, 0)
    calls = len(lib.calls)
    with pytest.raises(ValueError):
        eng.fanout_host_fec(*host, fec=fec[:2], members=members)
    assert len(lib.calls) == calls

    t = lambda ptr, nbytes, item=4: Tensor(ptr, nbytes, item)
    dev = (7, t(0x1000, 64, 1), t(0x2000, 4 * m), t(0x3000, 4 * m), t(0x4000, 4 * m), t(0x5000, 4 * n),
           t(0x6000, 192, 1), t(0x7000, 4 * n), t(0x8000, 4 * n), t(0x9000, 4 * n), t(0xA000, 4 * n))
    d_fec, d_mem, d_out = t(0xD000, 12 * n, 1), t(0xE000, 8), t(0xF000, n, 1)
    eng.fanout_device_fec(*dev, None, None, None, None, None, d_fec, d_mem, d_out)
    name, count, args = last()
    assert (name, count) == ("srtp_fanout_device_fec", 27)
    assert args[:6] == (0x1234, 0x1000, 0x2000, 0x3000, 0x4000, None) and args[6] == m
    assert args[7:10] == (0x5000, None, 7) and args[10:14] == (0x6000, 0x7000, 0x8000, 0x9000)
    assert args[14:] == (None, None, None, None, None, None, 0xD000, 0xE000, 2, 0xF000, 0xA000, n, None)
    eng.fanout_device_fec(*dev, None, None, None, None, None, None, None, None)
    assert last()[2][20:24] == (None, None, 0, None)
    calls = len(lib.calls)
    for bad in ((t(0xD000, 12 * n - 1, 1), d_mem, d_out), (d_fec, d_mem, t(0xF000, n - 1, 1))):
        with pytest.raises(ValueError):
            eng.fanout_device_fec(*dev, None, None, None, None, None, *bad)
    with pytest.raises(ValueError):
        eng.fanout_device_fec(*dev, None, None, None, None, None, d_fec, d_mem, d_out, n_members=3)
    assert len(lib.calls) == calls


def test_fan_out_fec_arithmetic_and_one_host_call(monkeypatch):
    """fan_out_fec shifts the media packets' sequence numbers by nb_fec, closes a group after every ``rate``
    packets and the open one at the end of the call, keeps counter and nb_fec across calls, lays the FEC entries
    out behind the media entries and reaches fanout_host_fec once."""
    import libjitsi_amd.srtp as S
    from libjitsi_amd import FecSender, RawPacket, fan_out_fec
    seen = []

    class Eng(S.SRTPEngine):
        trailer_room = 10

        def __init__(self):
            pass

        def fanout_host_fec(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap, src_status=None,
                            flags=None, rewrite=None, stamp=None, pay=None, red=None, fec=None, members=None):
            seen.append(dict(tid=np.array(tid), cap=np.array(cap), rewrite=None if rewrite is None else rewrite.copy(),
                             red=red, fec=fec, members=members, src_idx=np.array(src_idx), flags=np.array(flags)))
            n = len(off)
            fo = np.zeros(n, np.int8) if fec is None else (fec["mode"] != 0).astype(np.int8)
            st = np.where(fo == 1, 0, N.STATUS_SKIPPED).astype(np.int32)
            return np.full(n, 30, np.uint32), st, np.zeros(n, np.int8), fo

    eng = Eng()

    class T:
        packetPredicate = None

        def __init__(self, tid):
            self.engine, self.tid = eng, tid

    ts = [T(3), T(4), T(5)]
    A, B = 0x0A0A0A0A, 0x0B0B0B0B
    pk = [RawPacket(RG.packet(A if i != 2 else B, (0xFFFC + i) & 0xFFFF if i != 2 else 7, 40 + i), 0, 40 + i) for i in range(7)]
    s1, s2 = FecSender(A, 4, 116), FecSender(0x0C0C0C0C, 2, 117, 96)
    rw2 = lambda p: {"ssrc": 0x0C0C0C0C, "seq": 1000 + p.getSequenceNumber() % 16} if p.getSSRC() == A else {}
    out, codes, fec = fan_out_fec(pk, ts, [None, None, rw2], [None] * 3, [None] * 3, [None] * 3, [s1, None, s2])
    assert len(seen) == 1
    c = seen[0]
    T3, n0 = 3, 21
    # toward transformer 0: the six packets of SSRC A at rate 4: one full group, one closed short
    # toward transformer 2: the same six under the rewritten SSRC at rate 2: three groups
    assert len(c["cap"]) == n0 + 5 and c["src_idx"][n0:].tolist() == [-1] * 5 and c["tid"][n0:].tolist() == [3, 3, 5, 5, 5]
    a_idx = [i for i in range(7) if i != 2]
    assert c["fec"]["mode"].tolist() == [0] * n0 + [1, 1, 2, 2, 2]
    assert c["fec"]["count"][n0:].tolist() == [4, 2, 2, 2, 2] and c["fec"]["first"][n0:].tolist() == [0, 4, 6, 8, 10]
    assert c["fec"]["ssrc"][n0:].tolist() == [A, A, 0x0C0C0C0C] * 1 + [0x0C0C0C0C] * 2
    assert c["fec"]["pt"][n0:].tolist() == [116, 116, 117, 117, 117] and c["fec"]["red_pt"][n0:].tolist() == [0, 0, 96, 96, 96]
    assert c["members"].tolist() == [i * T3 for i in a_idx] + [i * T3 + 2 for i in a_idx]
    seq = lambda i: int.from_bytes(pk[i].data()[2:4], "big")
    rw = c["rewrite"]
    for pos, i in enumerate(a_idx):  # the shift: packets behind the first group's FEC packet move by one
        assert rw["mask"][i * T3] == N.REWRITE_SEQ and rw["seq"][i * T3] == (seq(i) + (pos >= 4)) & 0xFFFF
        assert rw["mask"][i * T3 + 2] == N.REWRITE_SSRC | N.REWRITE_SEQ
        assert rw["seq"][i * T3 + 2] == 1000 + seq(i) % 16 + pos // 2
    assert rw["mask"][2 * T3] == 0 and rw["mask"][1:n0:T3].tolist() == [0] * 7 and len(rw) == n0 + 5  # another SSRC; a peer without a sender
    # room for the longest member's copy less its 12 header bytes, the 27 of the FEC header, and the trailer
    assert c["cap"][n0:].tolist() == [54 + 15, 56 + 15, 51 + 15, 54 + 15, 56 + 15] and (c["flags"][n0:] == 0).all()
    assert (s1.counter, s1.nb_fec, s2.counter, s2.nb_fec) == (6, 2, 6, 3)
    assert [i for i, p in fec[0]] == [4, 6] and [i for i, p in fec[2]] == [1, 4, 6] and fec[1] == []
    assert all(p is not None and p.getLength() == 30 for k in (0, 2) for _, p in fec[k])
    assert codes == [[0] * 7] * 3 and out == [[None] * 7] * 3
    # the next call goes on from nb_fec; a group is not carried over
    fan_out_fec(pk[:1], ts, [None] * 3, [None] * 3, [None] * 3, [None] * 3, [s1, None, None])
    assert len(seen) == 2 and seen[1]["rewrite"]["seq"][0] == (seq(0) + 2) & 0xFFFF and (s1.counter, s1.nb_fec) == (7, 3)
    assert seen[1]["fec"]["count"].tolist() == [0, 0, 0, 1]
    # no sender at all: still one call through fanout_host_fec, with fec None
    fan_out_fec(pk[:2], ts, [None] * 3, [None] * 3, [None] * 3, [None] * 3, [None] * 3)
    assert len(seen) == 3 and seen[2]["fec"] is None and seen[2]["rewrite"] is None
    with pytest.raises(ValueError):
        fan_out_fec(pk, ts, [None] * 3, [None] * 3, [None] * 3, [None] * 3, [s1, None])
