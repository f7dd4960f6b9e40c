"""The entries the fan-out FEC tests run (tests/test_fanout_fec.py, on the GPU)
as plain data, so that a test without a GPU can hold every grid, by fec_ref
alone, to the result codes and counts the GPU tests assert.

A grid is a list of entries.  A media entry is red_grids' dict (its own source
packet, ``cap``, flags, the source's status, ``red``, ``rw``, ``ast``, ``pay``)
with ``fec`` None and ``peer``, an index into the test's peers.  An FEC entry
has ``fec``: a dict of ``members`` (indices of grid entries, in list order),
``ssrc``, ``pt``, ``red_pt``, ``mode`` and, for the refusals, ``count`` (the
record's count where it is not len(members)), ``overflow`` (the members stand
last in the members array and the count reaches past its end) and ``src`` (the
entry's own src_idx where it is not -1, a grid index).  ``cap`` None is the
packet and the trailer."""
import numpy as np

import abs_send_time_ref as A
import fec_ref as F
import payload_ref as P
import red_grids as RG
from libjitsi_amd import _native as N

SKIP = RG.SKIP
PLAIN, RED = 1, 2
FEC_PT, RED_PT = 116, 96
LISTS = ((12, 13, 14, 15, 16, 17, 27, 28, 29, 30, 43, 44, 45), (1008, 1009, 1010, 1011, 1012),
         (2032, 2033, 2034, 2035, 2036), (1200, 1200, 1200, 1200))

_ssrc = [0x0FEC0000]


def _next():
    _ssrc[0] += 1
    return _ssrc[0]


def media(pkt, peer=0, red=(RG.OFF, 0), **kw):
    e = RG.entry(pkt, red, **kw)
    e["fec"], e["peer"] = None, peer
    return e


def fec(members, mode=PLAIN, ssrc=None, pt=FEC_PT, red_pt=RED_PT, peer=0, cap=None, flags=0, **kw):
    rec = {"members": list(members), "ssrc": ssrc if ssrc is not None else _next(), "pt": pt, "red_pt": red_pt,
           "mode": mode, "count": None, "overflow": False, "src": None}
    assert not set(kw) - set(rec)
    rec.update(kw)
    return {"fec": rec, "cap": cap, "flags": flags, "peer": peer}


def media_cap(e, room):
    return e["cap"] if e["cap"] is not None else len(e["pkt"]) + 1 + room


def setters(b, r):
    """RawPacket's four setters on the bytearray b under the record r (mask, ssrc, ts, seq, pt)."""
    mask, ssrc, ts, seq, pt = (int(x) for x in tuple(r)[:5])
    if mask & N.REWRITE_PT:
        b[1] = (b[1] & 0x80) | (pt & 0x7F)
    if mask & N.REWRITE_SEQ:
        b[2:4] = (seq & 0xFFFF).to_bytes(2, "big")
    if mask & N.REWRITE_TIMESTAMP:
        b[4:8] = (ts & 0xFFFFFFFF).to_bytes(4, "big")
    if mask & N.REWRITE_SSRC:
        b[8:12] = (ssrc & 0xFFFFFFFF).to_bytes(4, "big")


def final(e, room):
    """A media entry as it stands in front of the protect chain: (bytes, len), or (None, 0) where it is skipped.
    bytes is None too where the copy is cut by its region (len > cap)."""
    result, b = RG.expect(e, room)
    if e["flags"] & SKIP or e["status"] != 0 or result < 0:
        return None, 0
    if len(b) > media_cap(e, room):
        return None, len(b)
    buf = bytearray(b)
    if len(buf) >= 12 and e["rw"] is not None:
        setters(buf, e["rw"])
    if e["pay"] is not None:
        P.apply(buf, e["pay"])
    if len(buf) >= 12 and e["ast"] is not None:
        A.apply(buf, e["ast"])
    return bytes(buf), len(buf)


def field_causes(grid, j):
    """The reasons the rule refuses FEC entry j for its record's fields or indices (the host route's EINVAL)."""
    r, n, why = grid[j]["fec"], len(grid), []
    count = r["count"] if r["count"] is not None else len(r["members"])
    if r["mode"] > 2:
        why.append("mode")
    if not 1 <= count <= 16:
        why.append("count")
    if r["overflow"]:
        why.append("first + count")
    if r["pt"] > 127 or (r["mode"] == 2 and r["red_pt"] > 127):
        why.append("pt")
    if r["src"] is not None:
        why.append("src_idx")
    for mi in r["members"][:max(count, 0)]:
        if not 0 <= mi < n:
            why.append("member index")
        elif grid[mi]["fec"] is not None and grid[mi]["fec"]["mode"] != 0:
            why.append("member record")
    return why


def expect(grid, room):
    """By fec_ref: (codes, packets, member_bytes).  codes[j] is 0, 1 or -1; packets[j] the plaintext of a made
    entry; member_bytes what the made entries XORed (len - 4 per member)."""
    codes, packets, member_bytes = [0] * len(grid), {}, 0
    for j, e in enumerate(grid):
        r = e["fec"]
        if r is None or r["mode"] == 0 or e["flags"] & SKIP:
            continue
        codes[j] = -1
        if field_causes(grid, j):
            continue
        got = [final(grid[mi], room) if grid[mi]["fec"] is None else (None, 0) for mi in r["members"]]
        if any(b is None or len(b) < 12 or (b[0] >> 6) != 2 for b, _ in got):
            continue
        codes[j] = 1
        packets[j] = F.make([b for b, _ in got], r["ssrc"], r["pt"], r["red_pt"] if r["mode"] == RED else None)
        member_bytes += sum(len(b) - 4 for b, _ in got)
    return codes, packets, member_bytes


def fec_cap(grid, j, room, packets):
    e = grid[j]
    return e["cap"] if e["cap"] is not None else (len(packets[j]) + room if j in packets else 64)


def arrays(grid):
    """(fec, members): the records of all n entries and the members array, each FEC entry's members in grid
    order, an overflowing entry's last."""
    rec = np.zeros(len(grid), N.FANOUT_FEC_DTYPE)
    order = [j for j, e in enumerate(grid) if e["fec"] is not None]
    order.sort(key=lambda j: grid[j]["fec"]["overflow"])
    members = []
    for j in order:
        r = grid[j]["fec"]
        count = r["count"] if r["count"] is not None else len(r["members"]) + (1 if r["overflow"] else 0)
        rec[j] = (len(members), r["ssrc"], count, r["pt"], r["red_pt"], r["mode"])
        members += r["members"]
    over = [j for j in order if grid[j]["fec"]["overflow"]]
    assert len(over) <= 1 and all(int(rec["first"][j]) + int(rec["count"][j]) > len(members) for j in over)
    return rec, np.array(members, np.int32)


# ---------------------------------------------------------------------- the grids
def refused_tail(g, peer=0):
    """One refused entry behind a grid of made ones: a group with a member the caller flagged."""
    at = len(g)
    g += stream((33, 34), peer=peer)
    g[at + 1]["flags"] = SKIP
    g.append(fec([at, at + 1], peer=peer))
    return g


def stream(lens, seq=100, ssrc=None, peer=0, **kw):
    """Consecutive media packets of one SSRC with the given lengths."""
    ssrc = ssrc if ssrc is not None else _next()
    return [media(RG.packet(ssrc, (seq + i) & 0xFFFF, c, pt=100, **kw), peer) for i, c in enumerate(lens)]


def boundaries(room):
    """Grid 1.  Every length list of LISTS as a group, plain and wrapped, into a destination that fits exactly,
    one without room for the trailer (ERR_CAPACITY) and one a byte short of the packet (DROP_INVALID); every
    length as the longest of a group of its own (itself and the list's shorter ones), so that the packet's end
    stands at every offset around a piece and, with 1008..1012, crosses byte 1024 -- lane 63's piece against lane
    0's second -- and with 2032..2036 byte 2048, the third trip; counts 1, 2, 3, 15 and 16; mixed lengths with
    the longest member first, in the middle and last; members with CSRCs and an extension."""
    g = []
    for lens in LISTS:
        at = len(g)
        g += stream(lens)
        idx = list(range(at, at + len(lens)))
        longest = max(lens) + 14
        for mode in (PLAIN, RED):
            size = longest + (mode == RED)
            for cap in (size + room, size, size - 1):
                g.append(fec(idx, mode, cap=cap))
            for i in range(len(lens)):
                g.append(fec(idx[:i + 1], mode))
    at = len(g)
    pool = [40 + (37 * i) % 90 for i in range(16)]
    g += stream(pool, seq=0xFFF8)  # the sequence numbers wrap inside the group
    for count in (1, 2, 3, 15, 16):
        for mode in (PLAIN, RED):
            g.append(fec(range(at, at + count), mode))
    for order in ((1200, 40, 77, 300, 13), (40, 77, 1200, 300, 13), (40, 77, 300, 13, 1200)):
        at = len(g)
        g += stream(order)
        g += [fec(range(at, at + 5), PLAIN), fec(range(at, at + 5), RED)]
    at = len(g)
    g += stream((60, 61, 90), cc=2, ext=RG.EL + bytes(8))
    g += [fec(range(at, at + 3), PLAIN), fec(range(at, at + 3), RED)]
    return refused_tail(g)


def with_records(room, peers=(0, 1)):
    """Grid 2.  Members that carry records: all four setters, a stamp, both payload patches, RED strip and wrap.
    The same four sources go toward two peers with different rewrites; each peer's group gets its own packet."""
    g, groups = [], []
    ssrc = _next()
    for k, peer in enumerate(peers):
        at = len(g)
        for i in range(4):
            base = RG.packet(ssrc, 500 + i, 120 + 7 * i, 0, RG.EL, pt=RG.RED_PT)
            rw = (0xF, 0x0FEC7000 + k, 0x01020304 + 960 * i + k, 0x2000 * (k + 1) + i, 0x60 + k, 0)
            kw = dict(rw=rw, ast=(0xC1D2E3 + i + 16 * k, 3, 1, 0), pay=(40, (0x31 + i, 0xB0 + (k if i == 0 else 0)), 21, (0x81, 0x82 + i)))  # one member's payload differs by peer
            red = ((RG.STRIP, RG.RED_PT), (RG.WRAP, RG.RED_PT), (RG.OFF, 0), (RG.STRIP, RG.RED_PT))[i]
            g.append(media(base, peer, red, **kw))
        groups.append(list(range(at, at + 4)))
    for k, peer in enumerate(peers):
        g.append(fec(groups[k], PLAIN, ssrc=0x0FEC7000 + k, peer=peer))
        g.append(fec(groups[k], RED, ssrc=0x0FEC7100 + k, peer=peer))
    return refused_tail(g, peers[0])


def field_refusals(made):
    """One FEC entry per cause the rule refuses for its record's fields or indices -- what the host route answers
    with SRTP_EINVAL.  Entries 0..3 of the grid are good members; ``made`` is an FEC entry."""
    return [fec([0, made]),                                         # a member's record is on
            fec([0, -1]), fec([0, 10 ** 6]),                        # a member names no entry
            fec([], count=0), fec(list(range(4)) * 4 + [0], count=17),
            fec([0, 1], pt=128), fec([0, 1], RED, red_pt=128), fec([0, 1], mode=3),
            fec([0, 1], src=2),                                     # its own src_idx names a source
            fec([2, 3], overflow=True)]                             # first + count > n_members


def refusals(room, device):
    """Grid 3.  One entry per refusal cause among entries that are made.  ``device``: the causes the host route
    answers with SRTP_EINVAL (fields and indices) are in; without it only those a running call can meet."""
    g = stream((50, 60, 70, 80))                                   # 0..3 good members
    g.append(media(RG.packet(_next(), 1, 64, pt=100), flags=SKIP))  # 4 flagged by the caller
    g.append(media(RG.packet(_next(), 1, 64, pt=100), status=4))    # 5 skipped by its source's status
    g.append(media(RG.packet(_next(), 1, 64, at_h=0x80 | RG.BLOCK_PT), red=(RG.STRIP, RG.RED_PT)))  # 6 dropped by RED
    g.append(media(RG.packet(_next(), 1, 64, pt=100), cap=40))      # 7 len > cap
    g.append(media(RG.packet(_next(), 1, 11, pt=100)))              # 8 len < 12
    g.append(media(RG.packet(_next(), 1, 64, pt=100, version=1)))   # 9 version 1
    g.append(fec([0, 1]))                                           # 10 made
    for mi in (4, 5, 6, 7, 8, 9):
        g.append(fec([0, mi, 1]))
    g.append(fec([2, 3], RED))                                      # made
    g.append(fec([0, 1], flags=SKIP))                               # the caller's SKIP: code 0
    if device:
        g.append(fec([0, 1], mode=0))                               # off: code 0, skipped by its source index
        made = len(g)
        g.append(fec([0, 1, 2]))                                    # made, and a member of the next
        g += field_refusals(made)
        g.append(fec([0, 1], PLAIN, red_pt=200))                    # made: red_pt is not looked at
    g.append(fec([1, 2, 3]))                                        # made, last
    return g


def shared(room):
    """Grid 4a.  Nine packets in three rows and three columns: six FEC entries, every packet in two of them."""
    g = stream([100 + 13 * i for i in range(9)])
    for r in range(3):
        g.append(fec([3 * r, 3 * r + 1, 3 * r + 2], PLAIN if r != 1 else RED))
    for c in range(3):
        g.append(fec([c, c + 3, c + 6], PLAIN if c != 1 else RED))
    return refused_tail(g)


def many(n_fec, per=2):
    """Grid 4b.  n_fec groups of ``per`` packets, each followed by its FEC entry."""
    g = []
    ssrc, fssrc = _next(), _next()
    for x in range(n_fec):
        at = len(g)
        g += stream([48 + (5 * x + i) % 40 for i in range(per)], seq=(per + 1) * x, ssrc=ssrc)
        g.append(fec(range(at, at + per), PLAIN if x % 3 else RED, ssrc=fssrc))
    return refused_tail(g)


def all_refused(room):
    """Grid 4c.  A call whose FEC entries are all refused: every media entry is flagged by the caller, so that
    no entry of the call reaches the chain."""
    g = [media(RG.packet(_next(), j, 40 + j, pt=100), flags=SKIP) for j in range(3)]
    return g + [fec([j % 3, (j + 1) % 3], PLAIN if j % 2 else RED) for j in range(5)]
