"""The entries the fan-out RED tests run (tests/test_fanout_red.py, on the GPU)
as plain data, so that a test without a GPU can hold every grid, by red_ref
alone, to carry each result code.  An entry is a dict: its own source packet
(``pkt``), the destination's capacity (``cap``; None: the packet, one byte for a
wrap and the trailer), the caller's flags, the source's status, and its records:
``red`` (mode, red_pt), and where present ``rw``, ``ast`` and ``pay`` as the
other fan-out tests spell them."""
import red_ref as R

OFF, STRIP, WRAP = R.OFF, R.STRIP, R.WRAP
RED_PT, BLOCK_PT = 96, 100
SKIP = 0x80000000
EL = b"\x32\xA0\xA1\xA2"  # abs-send-time, ID 3, len field 2
M32 = 0xFFFFFFFF


def packet(ssrc, seq, c, cc=0, ext=None, pt=RED_PT, marker=0, at_h=BLOCK_PT, version=2, ext_len=None):
    """An RTP packet of c bytes in all: cc CSRCs, a BEDE extension with the
    content ``ext`` (a multiple of 4 bytes; None: no X bit), the byte ``at_h``
    at the header's end where the packet reaches that far.  ``ext_len``
    overrides the two bytes of the extension's length word."""
    b = bytearray([(version << 6) | (0x10 if ext is not None else 0) | cc, (marker << 7) | pt])
    b += seq.to_bytes(2, "big") + (seq * 160 & M32).to_bytes(4, "big") + ssrc.to_bytes(4, "big")
    for i in range(cc):
        b += (0xC5C00000 + i).to_bytes(4, "big")
    if ext is not None:
        b += b"\xbe\xde" + (ext_len if ext_len is not None else (len(ext) // 4).to_bytes(2, "big")) + ext
    h = len(b)
    b += bytes((11 * i + 5 * seq + 1) & 0x7F for i in range(max(c - h, 0)))
    b = b[:c]
    if at_h is not None and h < c:
        b[h] = at_h
    return bytes(b)


def entry(pkt, red, cap=None, flags=0, status=0, rw=None, ast=None, pay=None, want=None):
    """want: the result code worked out by hand, where the grid states one."""
    return {"pkt": pkt, "red": red, "cap": cap, "flags": flags, "status": status, "rw": rw, "ast": ast, "pay": pay,
            "want": want}


def asked(e, room):
    """The packet's length when the step is asked for, else 0: not skipped, a mode, the whole packet there."""
    c = len(e["pkt"])
    cap = e["cap"] if e["cap"] is not None else c + 1 + room
    if e["flags"] & SKIP or e["status"] != 0 or e["red"][0] not in (STRIP, WRAP) or c < 12 or cap < c:
        return 0
    return c


def expect(e, room):
    """(result, bytes the later records see) by red_ref."""
    if not asked(e, room):
        return 0, e["pkt"]
    result, new = R.apply(e["pkt"], e["red"])
    return result, (new if result >= 0 else e["pkt"])


def codes(grid, room=16):
    return [expect(e, room)[0] for e in grid]


def malformed(e, room):
    """Whether the packet RED leaves has a version-2 header that ends outside it.  The protect chain answers
    ERR_MALFORMED there and, as the reference's loop ends with the exception, leaves the bundle's later entries
    NOT_PROCESSED: such entries stand last in a grid, so that every other entry runs through the chain."""
    result, b = expect(e, room)
    if result < 0 or e["flags"] & SKIP or e["status"] != 0 or len(b) < 12 or (b[0] >> 6) != 2:
        return False
    try:
        h = R.Pkt(b).header_length()
    except R.JavaThrow:
        return True
    return not 12 <= h <= len(b)


def malformed_last(grid, room):
    return [e for e in grid if not malformed(e, room)] + [e for e in grid if malformed(e, room)]


_ssrc = [0x0ED00000]


def _next():
    _ssrc[0] += 1
    return _ssrc[0]


HEADERS = [(0, None), (1, None), (0, EL), (1, EL), (0, EL + bytes(8)), (1, EL + bytes(8))]  # h = 12, 16, 20, 24, 28, 32


def boundaries(room):
    """Grid 1: h over 12..32, c at h, h + 1, around 32, 48, 1024 (lane 63's
    piece against lane 0's second) and 2048 (the second trip), both modes; wrap
    into a destination of c + 1 and of c bytes; strip of a 13-byte packet."""
    g = []
    for cc, ext in HEADERS:
        h = 12 + 4 * cc + (4 + len(ext) if ext is not None else 0)
        for c in sorted({h, h + 1, 31, 32, 33, 47, 48, 49, 1023, 1024, 1025, 2047, 2048, 2049}):
            if c < 12:
                continue
            for mode in (STRIP, WRAP):
                g.append(entry(packet(_next(), 7, c, cc, ext), (mode, RED_PT)))
    for c in (13, 40, 48, 64):
        g.append(entry(packet(_next(), 8, c), (STRIP, RED_PT)))
        g.append(entry(packet(_next(), 8, c), (WRAP, RED_PT), cap=c + 1))  # fits, without room for the trailer
        g.append(entry(packet(_next(), 8, c), (WRAP, RED_PT), cap=c))      # does not: DROP_INVALID
        g.append(entry(packet(_next(), 8, c), (WRAP, RED_PT), cap=c + 1 + room))
    g.append(entry(packet(_next(), 9, 64, at_h=0x80 | BLOCK_PT), (STRIP, RED_PT)))  # dropped
    g.append(entry(packet(_next(), 9, 64, pt=97), (STRIP, RED_PT)))                 # untouched
    return malformed_last(g, room)


KINDS = ("off", "strip", "wrap", "dropped", "source", "caller")


def _kind(kind, j):
    c = 40 + (7 * j) % 30
    if kind == "off":
        return entry(packet(_next(), j, c), (OFF, RED_PT))
    if kind == "strip":
        return entry(packet(_next(), j, c), (STRIP, RED_PT))
    if kind == "wrap":
        return entry(packet(_next(), j, c, pt=BLOCK_PT), (WRAP, RED_PT))
    if kind == "dropped":
        return entry(packet(_next(), j, c, at_h=0x80 | BLOCK_PT), (STRIP, RED_PT))
    if kind == "source":
        return entry(packet(_next(), j, c), (STRIP, RED_PT), status=4)
    return entry(packet(_next(), j, c), (WRAP, RED_PT), flags=SKIP)


def pairs(room):
    """Grid 2: every ordered pair of the six kinds in one wave's two entries, then one entry alone (n odd)."""
    g = []
    for a in KINDS:
        for b in KINDS:
            g.append(_kind(a, len(g)))
            g.append(_kind(b, len(g)))
    g.append(_kind("strip", len(g)))
    return g


def answers(room):
    """Grid 3: the reference's answers, one entry each (and a plain strip and wrap)."""
    P = lambda **kw: packet(_next(), 11, kw.pop("c", 60), **kw)
    S, W = (STRIP, RED_PT), (WRAP, RED_PT)
    T = lambda want, pkt, red: entry(pkt, red, want=want)
    return malformed_last([
        T(1, P(), S), T(2, P(pt=BLOCK_PT), W),
        T(-1, P(at_h=0x80 | BLOCK_PT), S),                      # multi-block
        T(-1, P(at_h=0xFF, c=200), S),                          # multi-block, the walk leaves the buffer
        T(0, P(pt=97), S),                                      # PT mismatch
        T(0, P(version=1), S), T(0, P(version=1), W),           # version 1
        T(0, P(pt=72, marker=1), (STRIP, 72)),                  # marker with PT 72..83
        T(0, P(pt=83, marker=1), (STRIP, 83)),
        T(1, P(pt=84, marker=1), (STRIP, 84)),                  # PT 84 with the marker is stripped
        T(2, P(pt=72, marker=1), (WRAP, 72)),                   # wrap has no predicate
        T(-1, P(c=20, ext=EL), S),                              # strip with h == c
        T(2, P(c=20, ext=EL), W),                               # wrap with h == c
        T(0, P(c=16, cc=2), S), T(-1, P(c=16, cc=2), W),        # h > c
        T(0, P(ext=EL, ext_len=b"\x80\x00"), S),                # a negative extension length
        T(-1, P(ext=EL, ext_len=b"\x80\x00"), W),
        T(0, P(ext=EL, ext_len=b"\x7F\xFF"), S), T(-1, P(ext=EL, ext_len=b"\x7F\xFF"), W),
        T(-1, P(c=15, ext=EL), S), T(-1, P(c=15, ext=EL), W),   # the length word past c
        T(-1, P(c=14, cc=1, ext=EL), S),
        T(2, P(ext=EL, ext_len=b"\xFF\xFC"), W),                # h == 0: byte 1 of the new packet is the moved b0
        T(1, P(ext=EL, ext_len=b"\xFF\xFD"), S), T(2, P(ext=EL, ext_len=b"\xFF\xFD"), W),  # h == 4
        T(0, P(), (OFF, RED_PT)), T(0, P(), (STRIP, 0)), T(1, P(pt=0, at_h=0), (STRIP, 0)),
        T(1, P(c=1200, cc=1, ext=EL + bytes(4)), S), T(2, P(c=1200, cc=1, ext=EL + bytes(4), pt=BLOCK_PT), W),
    ], room)


def together(room):
    """Grid 4: one entry per mode carrying all four records.  The extension is
    one word that is not the stamp's; the stamp's element stands in the four
    bytes past the extension, which the reference's walk still reads (its kept
    quirk): the first payload bytes, as RED left them.  A patch at h and one
    across the piece boundary at 32; all four setters.  Then entries for the
    other result codes."""
    g = []
    other = b"\x52\x01\x02\x03"  # ID 5, len field 2
    for mode in (STRIP, WRAP):
        # h = 20.  strip: the RED header is byte 20 and the element behind it moves down to 20..23.
        # wrap: the new byte 20 is the block PT 0x32 -- ID 3, len field 2 -- so that the inserted byte itself
        # is read as the stamp's element.
        if mode == STRIP:
            p = bytearray(packet(_next(), 21, 100, 0, other))
            p[21:25] = EL
        else:
            p = bytearray(packet(_next(), 21, 100, 0, other, pt=0x32))
        rw = (0xF, _next(), 0x01020304, 0x0506 + mode, 0x6B, 0)  # an SSRC of its own: the peer sees each once
        ast = (0xC1D2E3, 3, 1, 0)
        # the patch at h keeps the element's ID and len (the walk reads the patched bytes) and changes byte 21,
        # which the stamp then overwrites; the second patch straddles pieces 1 and 2
        pay = (20, (0x32, 0xB0), 31, (0x81, 0x82))
        g.append(entry(bytes(p), (mode, RED_PT), rw=rw, ast=ast, pay=pay))
    g.append(entry(packet(_next(), 22, 100, at_h=0x80), (STRIP, RED_PT), rw=(0xF, 1, 2, 3, 4, 0), ast=(5, 3, 1, 0),
                   pay=(12, (1, 2), 0, (0, 0))))
    g.append(entry(packet(_next(), 22, 100, 0, EL, pt=97), (STRIP, RED_PT), rw=(0xF, 0x11, 0x22, 0x33, 0x44, 0),
                   ast=(0xA1B2C3, 3, 1, 0), pay=(20, (0x91, 0x92), 0, (0, 0))))
    return g
