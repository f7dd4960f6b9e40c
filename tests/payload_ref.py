"""The payload writes of ExtendedSequenceNumberInterval.rewriteRTP restated byte
by byte over a bytearray of exactly the copied bytes (a helper, not a conftest):

write_short   RawPacket.writeShort (RawPacket.java:1334-1337), which
              setOriginalSequenceNumber calls with getHeaderLength()
              (RawPacket.java:1018-1022): data >> 8 at off, data at off + 1.
rewrite_fec   rewriteFEC's two stores
              (ExtendedSequenceNumberInterval.java:383-384) with the precedence
              quirk: ``snRewritenBase & 0xff00 >> 8`` is ``snRewritenBase &
              0xff``, so both bytes are the low byte.
The per-byte bound: a byte at or past the end of the copy is not written (Java
would throw; the fan-out rule leaves that byte out and writes the other), and a
patch whose offset is below 12 is refused whole.  apply() is one record: patch
0, then patch 1."""

HEADER = 12


def put(buf, i, v):
    """One writeByte under the bound."""
    if 0 <= i < len(buf):
        buf[i] = v & 0xFF


def patch(buf, at, b0, b1):
    """Two bytes at at, at + 1; refused whole below byte 12."""
    if at >= HEADER:
        put(buf, at, b0)
        put(buf, at + 1, b1)


def write_short(buf, off, data):
    patch(buf, off, (data >> 8) & 0xFF, data & 0xFF)


def fec_bytes(sn):
    """(byte) (sn & 0xff00 >> 8), (byte) (sn & 0x00ff) as Java evaluates them: >> binds tighter than &."""
    return sn & (0xFF00 >> 8) & 0xFF, sn & 0x00FF & 0xFF


def rewrite_fec(buf, off, sn):
    b2, b3 = fec_bytes(sn)
    patch(buf, off + 2, b2, b3)


def apply(buf, rec):
    """rec = (at0, (b00, b01), at1, (b10, b11)), srtp_fanout_payload's fields."""
    at0, b0, at1, b1 = rec
    patch(buf, int(at0), int(b0[0]), int(b0[1]))
    patch(buf, int(at1), int(b1[0]), int(b1[1]))
    return buf
