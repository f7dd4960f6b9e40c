"""The fan-out call as seen without a GPU: the entry points agree between the
header, _native.py and the built library; a NULL engine is refused before any
device is touched; the Python mirrors have the documented signatures;
srtp_fanout_job (fanout_job.h, the text k_fanout compiles) agrees, over the
sweep of tools/fanout_check.cpp, with ten lines of Python that restate the
rule; tools/fanout_check builds and runs clean under AddressSanitizer + UBSan."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device", "srtp_fanout_host", "srtp_engine_fanout_stats")
SKIP = N.PKT_FLAG_SKIP
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def test_entry_points_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY + ("srtp_fanout_job",):
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_fanout_stats;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint64_t calls, sources, destinations, skipped, src_bytes_h2d;"
    assert [n for n, _ in N.FanoutStats._fields_] == ["calls", "sources", "destinations", "skipped", "src_bytes_h2d"]
    assert C.sizeof(N.FanoutStats) == 40
    # srtp_stats is a struct of its own and did not grow
    assert C.sizeof(N.Stats) == 8 * (2 + N.NUM_STATUS + 12)
    # the header says that the host destination segment is output only
    doc = re.sub(r"\s*\*\s*", " ", header[header.index("Fan-out: one packet to many peers"):
                                         header.index("int srtp_fanout_device(")])
    assert "OUTPUT ONLY" in doc and "every other byte of it is unspecified" in doc


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                None, p(i), n, None) == -1
    assert L.srtp_fanout_host(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                              p(w), None, p(i), n) == -1
    assert L.srtp_engine_fanout_stats(None, C.byref(N.FanoutStats())) == -1
    assert L.srtp_fanout_job(0, 1, 12, 16, 0, 16, 0, None) == -1


def test_python_mirrors():
    from libjitsi_amd import SRTPEngine, fan_out
    import libjitsi_amd.srtp as S
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                             "seg", "off", "length", "cap", "status", "src_status", "flags", "m", "n",
                                             "stream"]
    assert sig(SRTPEngine.fanout_host) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx", "seg",
                                           "off", "cap", "src_status", "flags"]
    assert sig(SRTPEngine.fanout_stats) == ["self"]
    assert sig(fan_out) == ["pkts", "transformers", "exclusion"]
    for name in ("src_status", "flags", "m", "n", "stream"):
        assert inspect.signature(SRTPEngine.fanout_device).parameters[name].default is None
    assert inspect.signature(fan_out).parameters["exclusion"].default is None
    assert "OutputDataStreamImpl.java:171-243" in S.fan_out.__doc__
    assert S.fan_out([], []) == [] and S.fan_out([None], []) == []


def rule(idx, m, L, sc, st, dc, fl):
    """fanout_job restated: (copy_bytes, len_out, flags_out, by_source)."""
    by_source = idx < 0 or idx >= m or st != 0
    if by_source or fl & SKIP:
        return 0, 0, fl | SKIP, int(by_source)
    if L < 0 or sc < 0 or dc < 0:
        return 0, L, fl, 0
    c = min(L, sc, dc, 65535)
    return (c + 15) & ~15, L, fl, 0


def sweep():
    lens = list(range(81)) + [c + d for c in (1024, 2048, 4096, 65535) for d in range(-17, 18) if c + d <= 65537]
    caps = [c + d for c in (0, 16, 64, 1024, 2048, 4096, 65535) for d in (-17, -16, -1, 0, 1, 16)
            if 0 <= c + d <= 65535]
    for L in lens:
        for sc in caps:
            for dc in (sc - 17, sc - 1, sc, sc + 1, sc + 16, 12, 65535):
                if dc >= 0:
                    for fl in (0, SKIP):
                        yield 1, 3, L, sc, 0, dc, fl
    for idx in (I32_MIN, -1, 0, 1, 2, 3, 4, I32_MAX):
        for m in (0, 1, 3, I32_MAX):
            for st in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, -1):
                for fl in (0, 2, 6, SKIP, SKIP | 4):
                    for L, c in ((0, 0), (8, 16), (12, 16), (17, 16), (1200, 1216), (65535, 65535), (1200, 0)):
                        yield idx, m, L, c, st, c, fl
    for L in (I32_MIN, -1, 65536, 70000, I32_MAX, 100):
        for sc in (I32_MIN, -1, 0, 100, 65535, 65536, I32_MAX):
            for dc in (I32_MIN, -1, 0, 100, 65535, 65536, I32_MAX):
                yield 0, 1, L, sc, 0, dc, 0


def test_fanout_job_agrees_with_the_rule():
    job = N.lib().srtp_fanout_job
    out = N.FanoutPlan()
    ref = C.byref(out)
    cases = 0
    for case in sweep():
        assert job(*case, ref) == 0
        got = (out.copy_bytes, out.len_out, out.flags_out, out.by_source)
        assert got == rule(*case), (case, got, rule(*case))
        copy, (idx, m, L, sc, st, dc, fl) = got[0], case
        if copy:  # never past either region rounded up to 16
            assert copy % 16 == 0 and copy <= ((min(sc, 65535) + 15) & ~15) and copy <= ((min(dc, 65535) + 15) & ~15)
        cases += 1
    assert cases > 100000


def test_fanout_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_check (the Makefile's recipe, built out of tree): the rule
    swept and every copy replayed between exact-size heap buffers, a program of
    its own under AddressSanitizer + UBSan."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_check: fanout_check\.cpp .*fanout_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_check: \d+ cases, \d+ copies replayed, 0 failures", r.stdout)
