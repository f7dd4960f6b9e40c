"""FEC recovery on the device (srtp_fec_recover_device / _host, k_fec_recover,
FecReceiver): the grids of tests/fec_rx_grids.py on both routes against
FECReceiver.Reconstructor restated (tests/fec_rx_ref.py) -- bit equality on the
code, the length, the status and the bytes of every record, every other byte of
the output segment and the whole input segment untouched, and the counters;
what both routes refuse; receive -> recover -> forward on one stream with no
synchronise in between; and the Python mirror against the restated
FECReceiver over a scripted stream."""
import numpy as np
import pytest

import fec_ref as F
import fec_rx_grids as FG
import fec_rx_ref as R
import gcm_ref as G
from libjitsi_amd import FecReceiver, FecSender, RawPacket, fan_out_fec
from libjitsi_amd import _native as N
from oracle import oracle as O
from test_fanout import RTP, Peer, make_engine, seed, up16

pytestmark = pytest.mark.gpu

CODES = ("recovered", "complete", "waiting", "partial", "refused")


@pytest.fixture(scope="module")
def eng(engine_factory, oracle):
    return make_engine(engine_factory)


def d(a):
    import torch
    if a.dtype.names:
        a = a.view(np.uint8)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run(eng, grid, route):
    """One call over the grid: (out_seg, out_off, out_cap, out_len, out_status, code), the input segment held
    unchanged on the device route."""
    seg, off, ln, cap, status = FG.tables(grid)
    rec, cand, out_off, out_cap, out_bytes = FG.arrays(grid)
    if route == "host":
        out_seg = np.full(out_bytes, FG.FILL, np.uint8)
        before = seg.copy()
        out_len, out_status, code = eng.fec_recover_host(seg, off, ln, cap, rec, cand, out_seg, out_off, out_cap,
                                                         status=status)
        assert np.array_equal(seg, before)
        return out_seg, out_off, out_cap, out_len, out_status, code
    import torch
    t_seg, t_out = d(seg), torch.full((out_bytes,), FG.FILL, dtype=torch.uint8, device="cuda")
    t_len = torch.full((len(rec),), -1, dtype=torch.int32, device="cuda")
    t_st = torch.full((len(rec),), -1, dtype=torch.int32, device="cuda")
    t_code = torch.full((len(rec),), 0x55, dtype=torch.int8, device="cuda")
    args = (d(off), d(ln), d(cap), d(status), d(rec), d(cand), t_out, d(out_off), d(out_cap), t_len, t_st, t_code)
    torch.cuda.synchronize()
    s = eng.stream_ptr
    eng.fec_recover_device(t_seg, *args, stream=s)
    eng.sync(s)
    torch.cuda.synchronize()
    assert np.array_equal(t_seg.cpu().numpy(), seg)  # the input segment is never written
    return (t_out.cpu().numpy(), out_off, out_cap, t_len.cpu().numpy().view(np.uint32), t_st.cpu().numpy(),
            t_code.cpu().numpy())


def held(eng, name, route):
    """The grid on the route, held to the reference, with the stats' deltas."""
    grid = FG.ALL[name]()
    before = eng.fec_recover_stats()
    got = run(eng, grid, route)
    after = eng.fec_recover_stats()
    FG.check_outputs(grid, *got)
    c = FG.counts(grid)
    assert c == FG.COUNTS[name]
    delta = {k: after[k] - before[k] for k in after}
    print(name, route, "stats delta", delta)
    want = dict(zip(CODES, c[1:6]), calls=1, records=c[0] - c[6], member_bytes=FG.member_bytes(grid))
    assert delta == want
    return grid, got


ROUTES = ["host", "device"]


@pytest.mark.parametrize("route", ROUTES)
def test_boundaries(eng, route):
    """Needed counts 0 .. 47 at header lengths 12 / 16 / 20 / 24 under both masks, member lengths around every
    piece boundary up to 2036 (the second trip of the stride loop), the lost packet longer and shorter than the
    others, output regions one byte short (DROP_INVALID, the length kept), exact and roomy."""
    grid, (out_seg, out_off, out_cap, out_len, out_status, code) = held(eng, "boundaries", route)
    short = [r for r in range(len(code)) if code[r] == 1 and out_cap[r] == out_len[r] - 1]
    assert len(short) >= 10 and all(out_status[r] == N.STATUS_DROP_INVALID for r in short)
    assert {int(v) for v in out_len[code == 1]} >= {12, 13, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1200, 2036}
    assert (out_status[code != 1] == N.STATUS_SKIPPED).all() and (out_len[code != 1] == 0).all()


@pytest.mark.parametrize("route", ROUTES)
def test_mixed(eng, route):
    """63 candidates of which 60 lie outside the mask, duplicates in front of and behind the true packet,
    candidates whose status is not OK or whose len is below 12 or above cap, records that share their candidates,
    sparse long masks, and both outcomes of the wrap quirk."""
    held(eng, "mixed", route)


@pytest.mark.parametrize("route", ROUTES)
def test_many(eng, route):
    """126 records as a receiver makes them: every FEC packet of a stream with the stream's last entries as its
    candidates (up to 60, most of them shared with the records around it)."""
    held(eng, "many", route)


@pytest.mark.parametrize("route", ROUTES)
def test_refusals(eng, route):
    """Every cut of the FEC packet's header and payload, an extension length past the packet, a negative one, a FEC
    entry that does not count; on the device route also count > 64, first + count > n_cand, a FEC index out of
    range (refused) and candidate indices out of range (absent)."""
    held(eng, "refusals_" + route, route)


@pytest.mark.parametrize("route", ROUTES)
def test_all_refused(eng, route):
    """Not one record recovers: not one byte of the output segment is written."""
    grid, (out_seg, *_) = held(eng, "all_refused", route)
    assert (out_seg == FG.FILL).all()


def test_host_refuses_what_the_rule_would(eng):
    """SRTP_EINVAL with nothing launched: each record of the device route's grid that carries a cause, alone; a
    region outside its segment, an offset that is not aligned, and a capacity above 65535."""
    grid = FG.refusals(True)
    bad = [r for r in range(len(grid["records"])) if FG.field_causes(grid, r)]
    assert len(bad) == 9
    before = eng.fec_recover_stats()
    seg, off, ln, cap, status = FG.tables(grid)
    for r in bad:
        one = dict(entries=grid["entries"], records=[grid["records"][r]])
        rec, cand, out_off, out_cap, out_bytes = FG.arrays(one)
        if grid["records"][r]["first"] is None:  # the padding in front would make every index refusable
            rec["first"], cand = 0, cand[3:]
        out_seg = np.full(out_bytes, FG.FILL, np.uint8)
        with pytest.raises(N.SrtpError):
            eng.fec_recover_host(seg, off, ln, cap, rec, cand, out_seg, out_off, out_cap, status=status)
        assert (out_seg == FG.FILL).all()
    good = dict(entries=grid["entries"], records=[grid["records"][0]])
    rec, cand, out_off, out_cap, out_bytes = FG.arrays(good)
    out_seg = np.full(out_bytes, FG.FILL, np.uint8)
    for what in ("off", "cap", "end", "out_off", "out_end"):
        o, c, oo, osg = off.copy(), cap.copy(), out_off.copy(), out_seg
        if what == "off":
            o[3] += 4
        elif what == "cap":
            c[3] = 65536
        elif what == "end":
            o[-1] = len(seg) - 16
        elif what == "out_off":
            oo[0] += 8
        else:
            osg = out_seg[:-16]
        with pytest.raises(N.SrtpError):
            eng.fec_recover_host(seg, o, ln, c, rec, cand, osg, oo, out_cap, status=status)
    rec["on"] = 0  # a record that is off is not looked at
    rec["count"], rec["fec"] = 200, -9
    _, st, code = eng.fec_recover_host(seg, off, ln, cap, rec, cand, out_seg, out_off, out_cap, status=status)
    assert (code.tolist(), st.tolist()) == ([0], [N.STATUS_SKIPPED]) and (out_seg == FG.FILL).all()
    after = eng.fec_recover_stats()
    assert after["calls"] == before["calls"] + 1 and after["records"] == before["records"]


def test_record_alignment(eng):
    """rec and cand that are not 4-byte aligned: SRTP_EINVAL before any launch."""
    import torch
    grid = FG.all_refused()
    seg, off, ln, cap, status = FG.tables(grid)
    rec, cand, out_off, out_cap, out_bytes = FG.arrays(grid)
    n = len(rec)
    raw_rec = torch.zeros(16 * n + 8, dtype=torch.uint8, device="cuda")
    raw_cand = torch.zeros(4 * len(cand) + 8, dtype=torch.uint8, device="cuda")
    raw_rec[2:2 + 16 * n] = d(rec)
    raw_cand[2:2 + 4 * len(cand)] = d(cand.view(np.uint8))
    out = torch.full((out_bytes,), FG.FILL, dtype=torch.uint8, device="cuda")
    t_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t_code = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    before = eng.fec_recover_stats()
    common = (d(seg), d(off), d(ln), d(cap), d(status))
    tail = (out, d(out_off), d(out_cap), t_len, t_st, t_code)
    for r, c in ((raw_rec[2:2 + 16 * n], d(cand)), (d(rec), raw_cand[2:2 + 4 * len(cand)])):
        with pytest.raises(N.SrtpError):
            eng.fec_recover_device(*common, r, c, *tail, n_rec=n, n_cand=len(cand), stream=eng.stream_ptr)
    eng.sync(eng.stream_ptr)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FG.FILL).all() and (t_code.cpu().numpy() == 0x55).all()
    assert eng.fec_recover_stats() == before
    eng.fec_recover_device(*common, d(rec), d(cand), *tail, n_rec=0, stream=eng.stream_ptr)  # no record: nothing
    assert eng.fec_recover_stats() == before


@pytest.mark.parametrize("down", ["AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM"])
def test_receive_recover_forward_on_device(eng, down):
    """A sender protects groups of four plus FEC (fan_out_fec).  One media packet of each of six groups is
    withheld, one group arrives whole, one lacks two.  On one stream, with one synchronise at the end:
    transform_device(reverse), fec_recover_device with records built from the clear headers alone, fanout_device
    with the recovery's output arrays as sources to two peers.  Each peer's receiver, in the oracle and in the
    engine, gets the withheld packet's plaintext back."""
    import torch
    SSRC, PT = 0x0FEC0001, 116
    up, downs = seed(), [seed(), seed()]
    snd = Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", up)
    rcv = Peer([eng], RTP, "AES_CM_128_HMAC_SHA1_80", up, sender=False)  # the bridge: the same keys
    peers = [Peer([eng], RTP, down, k) for k in downs]
    rng = np.random.default_rng(5109 + len(down))
    clear = [FG.packet(rng, 0x7FE0 + i, int(rng.integers(40, 300)), pt=96) for i in range(32)]
    clear = [b"\x80" + c[1:8] + SSRC.to_bytes(4, "big") + c[12:] for c in clear]
    out, codes, fec = fan_out_fec([RawPacket(c, 0, len(c)) for c in clear], [snd.e[0]], [None], [None], [None],
                                  [None], [FecSender(SSRC, 4, PT)])
    assert len(fec[0]) == 8 and all(p is not None for _, p in fec[0])
    behind = dict(fec[0])
    wire, group_of = [], []
    for i in range(32):
        wire.append(out[0][i].data())
        group_of.append(i // 4)
        if i in behind:
            wire.append(behind[i].data())
            group_of.append(i // 4)
    assert len(wire) == 40
    # what the sender sent in the clear, by the oracle's receiver over the whole stream
    a_seg, a_off, a_len, a_cap = G.pack(wire, room=0)
    assert O.process(rcv.r, True, a_seg, a_off, a_len, a_cap).tolist() == [0] * 40
    plain = [a_seg[a_off[i]:a_off[i] + a_len[i]].tobytes() for i in range(40)]
    assert [p[1] & 0x7F for p in plain].count(PT) == 8
    # the loss: one media packet of groups 0..5 (a different place in each), none of group 6, two of group 7
    lost = {5 * g + (g % 4) for g in range(6)} | {5 * 7, 5 * 7 + 2}
    got_idx = [i for i in range(40) if i not in lost]
    w_seg, w_off, w_len, w_cap = G.pack([wire[i] for i in got_idx], room=0)
    n = len(got_idx)
    # records from the clear RTP headers alone: SSRC, payload type; every media entry of the SSRC is a candidate
    head = [wire[i][:12] for i in got_idx]
    media = [j for j, h in enumerate(head) if h[8:12] == SSRC.to_bytes(4, "big") and (h[1] & 0x7F) != PT]
    fecs = [j for j, h in enumerate(head) if (h[1] & 0x7F) == PT]
    assert len(fecs) == 8 and len(media) == 24
    rec = np.zeros(8, N.FEC_RECOVER_DTYPE)
    for r, j in enumerate(fecs):
        rec[r] = (j, 0, SSRC, len(media), 1, 0)
    cand = np.array(media, np.int32)
    out_cap = np.array([int(w_len[j]) for j in fecs], np.uint32)  # a recovered packet is shorter than its FEC packet
    out_off = np.zeros(8, np.uint32)
    out_off[1:] = np.cumsum([up16(c) for c in out_cap[:-1]])
    out_bytes = int(out_off[-1]) + up16(out_cap[-1])
    # the fan-out: record r's packet toward both peers
    idx = np.repeat(np.arange(8, dtype=np.int32), 2)
    tids = np.tile(np.array([p.tid for p in peers], np.int32), 8)
    f_cap = np.repeat(out_cap, 2) + 24
    f_off = np.zeros(16, np.uint32)
    f_off[1:] = np.cumsum([up16(c) for c in f_cap[:-1]])
    f_bytes = int(f_off[-1]) + up16(f_cap[-1])
    full = lambda k, v, dt: torch.full((k,), v, dtype=dt, device="cuda")
    r_seg, r_off, r_len, r_cap, r_st = d(w_seg), d(w_off), d(w_len), d(w_cap), full(n, -1, torch.int32)
    t_rec, t_cand, x_seg = d(rec), d(cand), full(out_bytes, FG.FILL, torch.uint8)
    x_off, x_cap, x_len, x_st, x_code = d(out_off), d(out_cap), full(8, -1, torch.int32), full(8, -1, torch.int32), full(8, 0x55, torch.int8)
    o_seg, o_len, o_st = full(f_bytes, FG.FILL, torch.uint8), full(16, -1, torch.int32), full(16, -1, torch.int32)
    o_idx, o_tids, o_off, o_cap = d(idx), d(tids), d(f_off), d(f_cap)
    s = eng.stream_ptr
    torch.cuda.synchronize()
    eng.transform_device(True, rcv.e[0].tid, r_seg, r_off, r_len, r_cap, r_st, stream=s)
    eng.fec_recover_device(r_seg, r_off, r_len, r_cap, r_st, t_rec, t_cand, x_seg, x_off, x_cap, x_len, x_st, x_code,
                           stream=s)
    eng.fanout_device(o_tids, x_seg, x_off, x_len, x_cap, o_idx, o_seg, o_off, o_len, o_cap, o_st, src_status=x_st,
                      stream=s)
    eng.sync(s)
    torch.cuda.synchronize()
    assert r_st.cpu().numpy().tolist() == [0] * n
    assert x_code.cpu().numpy().tolist() == [1] * 6 + [2, 3]
    assert x_st.cpu().numpy().tolist() == [0] * 6 + [9, 9]
    st = o_st.cpu().numpy()
    assert st.tolist() == [0] * 12 + [9] * 4
    withheld = [plain[5 * g + (g % 4)] for g in range(6)]
    xs, xl = x_seg.cpu().numpy(), x_len.cpu().numpy()
    for g in range(6):  # on the bridge: the plaintext, never on the host before now
        assert xs[out_off[g]:out_off[g] + xl[g]].tobytes() == withheld[g]
    o_seg_h, o_len_h = o_seg.cpu().numpy(), o_len.cpu().numpy().view(np.uint32).copy()
    for k, p in enumerate(peers):  # each peer's receiver, the oracle's and the engine's
        rx = Peer([eng], RTP, down, downs[k], sender=False)
        js = [2 * g + k for g in range(6)]
        sub_off, sub_cap = np.ascontiguousarray(f_off[js]), np.ascontiguousarray(f_cap[js])
        for proc in ("oracle", "engine"):
            seg_c, ln_c = o_seg_h.copy(), np.ascontiguousarray(o_len_h[js])
            if proc == "engine":
                got = eng.transform_host(True, rx.e[0].tid, seg_c, sub_off, ln_c, sub_cap)
            else:
                got = (G.process if rx.gcm else O.process)(rx.r, True, seg_c, sub_off, ln_c, sub_cap)
            assert np.asarray(got).tolist() == [0] * 6, (k, proc)
            for g in range(6):
                assert seg_c[sub_off[g]:sub_off[g] + ln_c[g]].tobytes() == withheld[g], (k, proc, g)


def test_fec_receiver_against_the_reference(eng):
    """FecReceiver.reverse_transform against fec_rx_ref.FECReceiver over a scripted stream with loss, reordering,
    a cascade (two FEC packets of which the second needs the first's recovery), buffer eviction and a wrap."""
    rng = np.random.default_rng(319)
    SSRC, PT = 0xFEC00319, 116
    mine, ref = FecReceiver(SSRC, PT, engine=eng), R.FECReceiver(SSRC, PT)
    seq = 65536 - 150
    stream = []
    for g in range(60):  # groups of four and their FEC packet, sequence numbers that wrap
        media = [FG.packet(rng, seq + i, int(rng.integers(12, 200)), pt=96) for i in range(4)]
        fec = bytearray(F.make(media, SSRC, PT))
        seq += 5
        drop = {0: [1], 1: [], 2: [0, 3], 3: [2], 4: [3]}[g % 5]
        stream += [m for i, m in enumerate(media) if i not in drop] + [bytes(fec)]
    # a cascade in one call: the second FEC packet (long mask, over one packet of the first group and one more)
    # lacks the packet the first one recovers, and one of its own
    base = (seq + 100) & 0xFFFF
    m = [FG.packet(rng, base + i, 60 + i, pt=96) for i in range(6)]
    f1 = F.make(m[:4], SSRC, PT)                                     # sequence number base + 4
    f2 = bytearray(FG.make_fec(rng, [m[1], m[5]], [0, 4], base + 1, 16, True, pt=PT))
    f2[2:4] = ((base + 6) & 0xFFFF).to_bytes(2, "big")
    cascade = [bytes(f2), m[0], m[2], m[3], f1]                      # m[1] and m[5] are lost; f1 is asked first
    calls = [stream[i:i + 7] for i in range(0, len(stream), 7)]
    calls[3] = calls[3][::-1]                                         # reordering inside a call
    calls[5], calls[6] = calls[6], calls[5]                           # and between calls
    calls.append(cascade)
    calls.append([None, None])
    rp = lambda b: None if b is None else RawPacket(b"\0\0" + b, 2, len(b))
    for c, batch in enumerate(calls):
        got = mine.reverse_transform([rp(b) for b in batch])
        want = ref.reverse_transform(batch)
        assert [None if p is None else p.data() for p in got] == want, c
        assert (mine.nb_fec, mine.nb_recovered) == (ref.nb_fec, ref.nb_recovered), c
        assert sorted(mine.fec) == sorted(ref.fecs) and mine.media == ref.media, c
    assert ref.nb_recovered >= 30 and len(ref.media) == 64 and ref.nb_fec == 60 + 2
    assert [R.seq_of(p) for p in want if p is not None] == []          # nothing more to recover
    last = ref.reverse_transform([])                                    # the cascade recovered both
    assert {(base + 1) & 0xFFFF, (base + 5) & 0xFFFF} <= set(ref.media) and last == []
