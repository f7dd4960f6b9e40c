"""The grids of the FEC recovery tests, shared by the CPU tests (which hold them
to tests/fec_rx_ref.py alone) and the GPU tests (which run them).

A grid is ``{"entries": [...], "records": [...]}``.  An entry is a received
packet: ``dict(data=bytes, len=None or an override, cap=None or an override,
status=0)``.  A record is ``dict(fec=entry index, cands=[entry indices], ssrc=,
on=1, out_cap=None or an override, first=None, count=None)``; ``first`` and
``count`` override what :func:`arrays` would lay out (the device route's
refusals)."""
import numpy as np

import fec_ref
import fec_rx_ref as R

ROOM = 8        # bytes of a region behind its packet
FILL = 0xEE     # what an output segment holds before a call
JUNK = 0x5A     # what lies between the regions of the input segment


def up16(v):
    return (v + 15) & ~15


def packet(rng, seq, length, pt=100):
    b = bytearray(rng.integers(0, 256, length, np.uint8).tobytes())
    b[0] = 0x80 | (b[0] & 0x2F)  # version 2, no extension
    if length > 1:
        b[1] = (b[1] & 0x80) | pt
    if length > 3:
        b[2:4] = (seq & 0xFFFF).to_bytes(2, "big")
    return bytes(b)


def make_fec(rng, media, pos, base, hl=12, long_mask=False, pt=116, plen=None):
    """An ulpfec packet (RFC 5109, one level) over ``media`` at mask positions ``pos``, behind an RTP header of
    ``hl`` bytes (12; 16: one CSRC; 20, 24: an extension of one or two words)."""
    want = max(len(m) - 12 for m in media)
    pay = hl + (18 if long_mask else 14)
    f = bytearray(pay + want)
    f[:hl] = rng.integers(0, 256, hl, np.uint8).tobytes()
    if hl == 12:
        f[0] = 0x80
    elif hl == 16:
        f[0] = 0x81
    else:
        f[0], f[14], f[15] = 0x90, 0, (hl - 16) // 4
    f[1] = pt
    lx = 0
    for m, k in zip(media, pos):
        for i in range(8):
            f[hl + i] ^= m[i]
        lx ^= len(m) - 12
        for i in range(12, len(m)):
            f[pay + i - 12] ^= m[i]
        f[hl + 12 + k // 8] |= 0x80 >> (k % 8)
    f[hl] = (f[hl] & ~0x40 & 0xFF) | (0x40 if long_mask else 0)
    f[hl + 2:hl + 4] = (base & 0xFFFF).to_bytes(2, "big")
    f[hl + 8:hl + 10] = lx.to_bytes(2, "big")
    f[hl + 10:hl + 12] = (want if plen is None else plen).to_bytes(2, "big")
    return bytes(f)


class Grid:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.entries, self.records = [], []

    def entry(self, data, **kw):
        self.entries.append(dict(data=bytes(data), len=kw.get("len"), cap=kw.get("cap"), status=kw.get("status", 0)))
        return len(self.entries) - 1

    def record(self, fec, cands, ssrc=None, **kw):
        ssrc = int(self.rng.integers(0, 1 << 32)) if ssrc is None else ssrc
        self.records.append(dict(fec=fec, cands=list(cands), ssrc=ssrc, on=kw.get("on", 1), out_cap=kw.get("out_cap"),
                                 first=kw.get("first"), count=kw.get("count")))
        return len(self.records) - 1

    def group(self, lens, lost=(), base=None, pos=None, hl=12, long_mask=False, extra=0, out_delta=None, plen=None,
              via_sender=False, cut=None, shuffle=True):
        """A protected group whose packets ``lost`` (indices) were not received, and its record."""
        rng = self.rng
        base = int(rng.integers(0, 60000)) if base is None else base
        pos = list(range(len(lens))) if pos is None else pos
        media = [packet(rng, base + k, n) for k, n in zip(pos, lens)]
        if via_sender:  # FECSender restated: consecutive members, the short mask, a header of 12
            fec = fec_ref.make(media, 0x1234, 116)
        else:
            fec = make_fec(rng, media, pos, base, hl, long_mask, plen=plen)
        if cut is not None:
            fec = fec[:cut]
        cands = [self.entry(packet(rng, base - 1 - int(rng.integers(0, 300)), int(rng.integers(12, 80))))
                 for _ in range(extra)]
        cands += [self.entry(m) for i, m in enumerate(media) if i not in lost]
        if shuffle:
            rng.shuffle(cands)
        f = self.entry(fec)
        out_cap = None
        if out_delta is not None:
            assert len(lost) == 1
            out_cap = len(media[lost[0]]) + out_delta
        return self.record(f, cands, out_cap=out_cap), media

    def every_code(self):
        """Records with each of the other codes, so that every grid holds all six."""
        self.group([40, 41, 42, 43], lost=[2], extra=3)                           # RECOVERED
        self.group([40, 41, 42, 43], extra=2)                                     # COMPLETE
        self.group([40, 41, 42, 43], lost=[0, 3], extra=2)                        # WAIT
        self.group([40, 90], lost=[1], plen=40)                                   # PARTIAL
        self.group([40, 60], lost=[1], cut=12 + 14 + 47)                          # REFUSED: the payload ends early
        r, _ = self.group([40, 41], lost=[1])
        self.records[r]["on"] = 0                                                 # OFF
        return self

    def done(self):
        return dict(entries=self.entries, records=self.records)


LENS = (12, 13, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45, 1200, 2036)
NEEDED = (0, 1, 3, 4, 5, 15, 16, 47)


def boundaries():
    """Every needed count at every header length, member lengths around every piece boundary, the lost packet
    longer and shorter than the others, and output regions one byte short, exact and roomy."""
    g = Grid(5109)
    i = 0
    for needed in NEEDED:
        for hl in (12, 16, 20, 24):
            long_mask = needed + 1 > 16 or (i % 2 == 1)
            n = LENS[i % len(LENS)]
            lens = [n] * (needed + 1)
            lost = i % (needed + 1)
            g.group(lens, lost=[lost], hl=hl, long_mask=long_mask, extra=(i * 7) % (64 - needed),
                    out_delta=(0, -1, ROOM)[i % 3])
            i += 1
    for n in LENS:  # the lost one alone decides the length: above and below every other member's
        others = [LENS[(LENS.index(n) + d) % len(LENS)] for d in (1, 5, 9)]
        g.group([n] + others, lost=[0], hl=(12, 16, 20, 24)[i % 4], long_mask=bool(i % 2), out_delta=(0, -1, ROOM)[i % 3])
        g.group(others + [n], lost=[1], via_sender=True, extra=5)
        i += 1
    g.group([1200] * 4, lost=[3], via_sender=True)
    return g.every_code().done()


def mixed():
    """64 candidates of which most lie outside the mask, duplicates, absent candidates, candidates shared between
    records, sparse long masks and the wrap quirk."""
    g = Grid(2198)
    rng = g.rng
    for k in range(6):
        r, media = g.group([60 + k, 200, 61, 35 + k], lost=[k % 4], extra=60, hl=(12, 20)[k % 2])
        assert len(g.records[r]["cands"]) == 63
    # duplicates: another packet under a member's number, in front of it (loses) and behind it (stands)
    for behind in (False, True):
        r, media = g.group([50, 50, 50], lost=[2], shuffle=False)
        rec = g.records[r]
        twin = g.entry(packet(rng, int.from_bytes(media[1][2:4], "big"), 50))
        rec["cands"] = rec["cands"] + [twin] if behind else [twin] + rec["cands"]
    # absent candidates: a status that is not OK, a length below 12, a length above the region
    for how in ("status", "short", "long"):
        r, media = g.group([44, 45, 46, 47], lost=[1], shuffle=False)
        e = g.entries[g.records[r]["cands"][0]]
        if how == "status":
            e["status"] = 2
        elif how == "short":
            e["len"] = 11
        else:
            e["cap"] = len(e["data"]) - 1
    # two records over one window of entries: a short and a long FEC packet over overlapping groups
    base = 40000
    media = [packet(rng, base + k, 30 + 3 * k) for k in range(12)]
    ids = [g.entry(m) for k, m in enumerate(media) if k not in (2, 9)]
    f1 = g.entry(make_fec(rng, media[:6], list(range(6)), base))
    f2 = g.entry(make_fec(rng, media[4:], list(range(8)), base + 4, hl=16, long_mask=True))
    f3 = g.entry(make_fec(rng, media, list(range(12)), base, long_mask=True))
    g.record(f1, ids)
    g.record(f2, ids)
    g.record(f3, ids)  # two missing
    # sparse long masks
    for k in range(4):
        pos = sorted(rng.choice(48, 9, replace=False).tolist())
        g.group([int(rng.integers(12, 300)) for _ in pos], lost=[k * 2], pos=pos, long_mask=True, hl=(12, 24)[k % 2],
                extra=20)
    # the wrap quirk: a complete group with one key past 65535 recovers a duplicate, with two it waits
    g.group([40, 41, 42, 43], base=65533)
    g.group([40, 41, 42, 43], base=65534)
    g.group([40, 41, 42, 43], base=65533, lost=[1])  # and one truly lost: two missing
    g.group([40, 41, 42, 43], base=65532, lost=[1])  # no key past the wrap
    return g.every_code().done()


def many(groups=120):
    """A few hundred records as a receiver makes them: groups of four and their FEC packet, every record with the
    stream's last entries as candidates."""
    g = Grid(3550)
    rng = g.rng
    for s in range(groups // 8):
        base = int(rng.integers(0, 65536 - 64))
        window = []
        for k in range(8):
            media = [packet(rng, base + 5 * k + i, int(rng.integers(12, 400))) for i in range(4)]
            lost = [int(rng.integers(0, 4))] if k % 3 == 0 else [0, 2] if k % 5 == 4 else []
            window += [g.entry(m) for i, m in enumerate(media) if i not in lost]
            f = g.entry(fec_ref.make(media, 7, 116))
            g.record(f, window[-60:])
    return g.every_code().done()


def refusals(device):
    """Every refusal.  The host route answers SRTP_EINVAL for a record's own fields and for indices out of
    range, so those are in the device route's grid only."""
    g = Grid(7714)
    rng = g.rng
    for hl in (12, 16, 20, 24):
        for long_mask in (False, True):
            pay = hl + (18 if long_mask else 14)
            for cut in (12, hl + 1, pay - 1, pay, pay + 27, pay + 28):  # the last one recovers
                g.group([40, 50], lost=[0], hl=hl, long_mask=long_mask, cut=max(cut, 12))
    # the extension length: past the packet, negative, and cut off
    r, _ = g.group([40, 50], lost=[0], hl=20)
    e = g.entries[g.records[r]["fec"]]
    e["data"] = e["data"][:14] + b"\x7f\xff" + e["data"][16:]
    r, _ = g.group([40, 50], lost=[0], hl=20)
    e = g.entries[g.records[r]["fec"]]
    e["data"] = e["data"][:14] + b"\x80\x00" + e["data"][16:]
    r, _ = g.group([40, 50], lost=[0], hl=20)
    e = g.entries[g.records[r]["fec"]]
    e["data"] = e["data"][:15]
    # the FEC entry itself does not count
    for how in ("status", "short", "long"):
        r, _ = g.group([40, 50], lost=[0])
        e = g.entries[g.records[r]["fec"]]
        if how == "status":
            e["status"] = 2
        elif how == "short":
            e["len"] = 11
        else:
            e["cap"] = len(e["data"]) - 1
    if device:
        r, _ = g.group([40, 50], lost=[0])
        g.records[r]["count"] = 65
        r, _ = g.group([40, 50], lost=[0])
        g.records[r]["first"] = 1 << 30
        r, _ = g.group([40, 50], lost=[0])
        g.records[r]["first"] = 0xFFFFFFFF
        for bad in (-1, "n", 1 << 30):
            r, _ = g.group([40, 50], lost=[0])
            g.records[r]["fec"] = bad
        for bad in (-1, "n", -(1 << 31)):  # a candidate index out of range is an absent candidate
            r, _ = g.group([40, 50, 60], lost=[0])
            g.records[r]["cands"][0] = bad
    return g.every_code().done()


def all_refused():
    g = Grid(6464)
    for hl in (12, 16, 20, 24):
        g.group([40, 50], lost=[0], hl=hl, cut=hl + 13)
        g.group([40, 50], lost=[0], hl=hl, long_mask=True, cut=hl + 17)
    r, _ = g.group([40, 41], lost=[1])
    g.records[r]["on"] = 0
    return g.done()


ALL = {"boundaries": boundaries, "mixed": mixed, "many": many, "refusals_host": lambda: refusals(False),
       "refusals_device": lambda: refusals(True), "all_refused": all_refused}
# grid: (records, recovered, complete, waiting, partial, refused, off) -- what the GPU tests assert
COUNTS = {
    "boundaries": (67, 62, 1, 1, 1, 1, 1), "mixed": (28, 17, 1, 7, 1, 1, 1), "many": (126, 46, 61, 16, 1, 1, 1),
    "refusals_host": (60, 9, 1, 1, 1, 47, 1), "refusals_device": (69, 9, 1, 4, 1, 53, 1),
    "all_refused": (9, 0, 0, 0, 0, 8, 1),
}


def resolve(grid, v):
    return len(grid["entries"]) if v == "n" else v


def entry_fields(e):
    n = len(e["data"]) if e["len"] is None else e["len"]
    cap = len(e["data"]) + ROOM if e["cap"] is None else e["cap"]
    return n, cap, e["status"]


def tables(grid):
    """The received tables: (seg, off, len, cap, status).  A region is the data rounded up to 16 plus slack."""
    es = grid["entries"]
    off, at = [], 0
    for e in es:
        off.append(at)
        at += up16(max(len(e["data"]) + ROOM, 16)) + 16 * (len(off) % 2)
    seg = np.full(at, JUNK, np.uint8)
    for e, o in zip(es, off):
        seg[o:o + len(e["data"])] = np.frombuffer(e["data"], np.uint8)
    f = [entry_fields(e) for e in es]
    return (seg, np.array(off, np.uint32), np.array([x[0] for x in f], np.uint32),
            np.array([x[1] for x in f], np.uint32), np.array([x[2] for x in f], np.int32))


def present(grid, i):
    """The entry's bytes where the rule counts it, else None."""
    i = resolve(grid, i)
    if not 0 <= i < len(grid["entries"]):
        return None
    e = grid["entries"][i]
    n, cap, status = entry_fields(e)
    if status != 0 or not 12 <= n <= cap <= 65535:
        return None
    return e["data"][:n]


def arrays(grid):
    """(rec, cand, out_off, out_cap, out_seg_bytes): the records laid out, candidates back to back (a few shared
    slots of padding in front), output regions roomy unless the record says otherwise."""
    want = expect(grid)
    rec = np.zeros(len(grid["records"]), _dtype())
    cand, out_off, out_cap, at = [0x7FFFFFFF, -5, 3], [], [], 0
    for r, (x, w) in enumerate(zip(grid["records"], want)):
        first = len(cand)
        cand += [resolve(grid, c) for c in x["cands"]]
        fi = resolve(grid, x["fec"])
        rec[r] = (fi, first if x["first"] is None else x["first"], x["ssrc"],
                  len(x["cands"]) if x["count"] is None else x["count"], x["on"], 0xBEEF)
        cap = (w[2] + ROOM if w[2] else 40) if x["out_cap"] is None else x["out_cap"]
        out_off.append(at)
        out_cap.append(cap)
        at += up16(max(cap, 1)) + 16 * (r % 3)
    return rec, np.array(cand, np.int32), np.array(out_off, np.uint32), np.array(out_cap, np.uint32), at


def _dtype():
    return np.dtype([("fec", "<i4"), ("first", "<u4"), ("ssrc", "<u4"), ("count", "u1"), ("on", "u1"),
                     ("reserved", "<u2")])


def field_causes(grid, r):
    """Why the host route would answer SRTP_EINVAL for record r (empty: it would not)."""
    x = grid["records"][r]
    n = len(grid["entries"])
    causes = []
    if not x["on"]:
        return causes
    if (x["count"] or 0) > 64 or len(x["cands"]) > 64:
        causes.append("count")
    if x["first"] is not None:
        causes.append("first + count")
    if not 0 <= resolve(grid, x["fec"]) < n:
        causes.append("fec index")
    if any(not 0 <= resolve(grid, c) < n for c in x["cands"]):
        causes.append("candidate index")
    return causes


def expect(grid):
    """By fec_rx_ref alone: per record (code, packet or None, out_len, out_status)."""
    out = []
    for r, x in enumerate(grid["records"]):
        if not x["on"]:
            out.append((R.OFF, None, 0, 9))
            continue
        causes = field_causes(grid, r)
        if "count" in causes or "first + count" in causes:
            out.append((R.REFUSED, None, 0, 9))
            continue
        code, pkt = R.one(present(grid, x["fec"]), [present(grid, c) for c in x["cands"]], x["ssrc"])
        if code != R.RECOVERED:
            out.append((code, None, 0, 9))
            continue
        cap = len(pkt) + ROOM if x["out_cap"] is None else x["out_cap"]
        out.append((code, pkt, len(pkt), 0 if len(pkt) <= cap else 7))
    return out


def counts(grid):
    codes = [w[0] for w in expect(grid)]
    return (len(codes),) + tuple(codes.count(c) for c in (R.RECOVERED, R.COMPLETE, R.WAIT, R.PARTIAL, R.REFUSED, R.OFF))


def member_bytes(grid):
    """What the kernel counts: len - 4 per needed member of a recovered record."""
    total = 0
    for x, w in zip(grid["records"], expect(grid)):
        if w[0] != R.RECOVERED:
            continue
        fec = present(grid, x["fec"])
        hl = R.header_length(fec)
        long_mask = bool(fec[hl] & 0x40)
        base = int.from_bytes(fec[hl + 2:hl + 4], "big")
        mask = int.from_bytes(fec[hl + 12:hl + (18 if long_mask else 14)], "big")
        bits = 48 if long_mask else 16
        media = {}
        for c in x["cands"]:
            p = present(grid, c)
            if p is not None:
                media[R.seq_of(p)] = p
        for k in range(bits):
            if mask >> (bits - 1 - k) & 1 and base + k in media:
                total += len(media[base + k]) - 4
    return total


def check_outputs(grid, out_seg, out_off, out_cap, out_len, out_status, code):
    """Bit equality with the reference on code, out_len, out_status and the bytes; every FILL byte outside the
    written regions rounded up to 16, and the whole region of every record that did not recover."""
    want = expect(grid)
    assert [int(c) for c in code] == [w[0] for w in want]
    assert [int(v) for v in out_len] == [w[2] for w in want]
    assert [int(v) for v in out_status] == [w[3] for w in want]
    untouched = np.ones(len(out_seg), bool)
    for r, w in enumerate(want):
        if w[0] != R.RECOVERED:
            continue
        o, cap = int(out_off[r]), int(out_cap[r])
        n = min(w[2], cap)
        assert bytes(out_seg[o:o + n]) == w[1][:n], r
        untouched[o:o + up16(n)] = False
    assert (out_seg[untouched] == FILL).all()
