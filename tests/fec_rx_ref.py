"""FECReceiver (transform/fec/FECReceiver.java) restated line by line over
Python bytes: ``Reconstructor`` is setFecPacket (:472-520) and recover
(:527-596) over a map of media packets, ``FECReceiver`` is reverseTransform
(:233-319) with saveFec (:350-356) and saveMedia (:364-389).

The restatement keeps what the Java does.  ``media.get(base + i * 8 + j)`` is
asked with an int that is not reduced mod 2^16, so a key above 65535 is never
found; the map is a TreeMap under seqNumComparator (:49-74), whose firstKey is
the oldest sequence number of a set that spans fewer than 2^15.

Two deviations are defined where the Java reads the stale bytes of a larger
buffer or throws: ``REFUSED`` when a read of the FEC packet would fall at or
past its length (the extension length of getHeaderLength, a negative header
length, hl + 14 or, with the long mask, hl + 18 greater than the length), and
``REFUSED`` when, for a recovery, payload start + lengthRecovery exceeds the
length."""
import functools

OFF, RECOVERED, COMPLETE, WAIT, PARTIAL, REFUSED = 0, 1, 2, 3, 4, -1
MEDIA_BUF_SIZE, FEC_BUF_SIZE = 64, 32


def sbyte(b):
    return b - 256 if b >= 128 else b


def header_length(p):
    """RawPacket.getHeaderLength (:602-614) over getExtensionLength (:544-556); None where a read leaves the packet."""
    h = 12 + 4 * (p[0] & 0x0F)
    if p[0] & 0x10:
        x = h + 2
        if x + 1 >= len(p):
            return None
        h += 4 + ((sbyte(p[x]) << 8) | p[x + 1]) * 4
    return h


def seq_of(p):
    return (p[2] << 8) | p[3]


def seq_cmp(a, b):
    """seqNumComparator (:49-74)"""
    if a == b:
        return 0
    if a > b:
        return 1 if a - b < 32768 else -1
    return -1 if b - a < 32768 else 1


def first_key(d):
    """TreeMap.firstKey under seqNumComparator, for a set that spans fewer than 2^15 sequence numbers."""
    return sorted(d, key=functools.cmp_to_key(seq_cmp))[0]


class Reconstructor:
    def __init__(self, media, ssrc):
        self.media, self.ssrc = media, ssrc  # media: {sequence number: bytes}
        self.needed, self.num_missing, self.sequence_number, self.fec = [], -1, -1, None
        self.refused = False

    def set_fec_packet(self, p):  # :472-520
        self.needed, self.num_missing, self.sequence_number, self.fec = [], 0, -1, bytes(p)
        self.refused = True
        buf = self.fec
        hl = header_length(buf) if len(buf) >= 12 else None
        if hl is None or hl < 0 or hl + 14 > len(buf):
            return  # the defined deviation
        mask_len = 2 if (buf[hl] & 0x40) == 0 else 6
        if mask_len == 6 and hl + 18 > len(buf):
            return
        self.refused = False
        base = (buf[hl + 2] << 8) | buf[hl + 3]
        idx = hl + 12
        done = False
        for i in range(mask_len):
            for j in range(8):
                if buf[idx + i] & (1 << (7 - j) & 0xFF):
                    pkt = self.media.get(base + i * 8 + j)
                    if pkt is not None:
                        self.needed.append(pkt)
                    else:
                        self.sequence_number = base + i * 8 + j
                        self.num_missing += 1
                if self.num_missing > 1:
                    done = True
                    break
            if done:
                break
        if self.num_missing != 1:
            self.sequence_number = -1

    def can_recover(self):
        return self.num_missing == 1

    def recover(self):  # :527-596 -> (code, bytes or None)
        if not self.can_recover():
            return None, None
        fec = self.fec
        idx = header_length(fec)
        length_recovery = (fec[idx + 8] << 8) | fec[idx + 9]
        for p in self.needed:
            length_recovery ^= len(p) - 12
        length_recovery &= 0xFFFF
        out = bytearray(length_recovery + 12)
        out[0:8] = fec[idx:idx + 8]
        for p in self.needed:
            for i in range(8):
                out[i] ^= p[i]
        out[0] &= 0x3F
        out[0] |= 0x80
        long_mask = (fec[idx] & 0x40) != 0
        idx += 10
        protection_length = (fec[idx] << 8) | fec[idx + 1]
        if protection_length < length_recovery:
            return PARTIAL, None
        idx += 4
        if long_mask:
            idx += 4
        if idx + length_recovery > len(fec):
            return REFUSED, None  # the defined deviation: System.arraycopy would throw or copy stale bytes
        out[12:12 + length_recovery] = fec[idx:idx + length_recovery]
        for p in self.needed:
            for i in range(12, min(length_recovery + 12, len(p))):
                out[i] ^= p[i]
        out[8:12] = (self.ssrc & 0xFFFFFFFF).to_bytes(4, "big")           # setSSRC((int) ssrc)
        out[2:4] = (self.sequence_number & 0xFFFF).to_bytes(2, "big")     # setSequenceNumber: two writeByte
        return RECOVERED, bytes(out)


def one(fec, candidates, ssrc):
    """One stateless record: ``candidates`` is the list of present packets (bytes of at least 12), the later of
    two with equal sequence numbers standing.  Returns (code, packet or None)."""
    if fec is None or not 12 <= len(fec) <= 65535:
        return REFUSED, None
    media = {}
    for c in candidates:
        if c is not None and 12 <= len(c) <= 65535:
            media[seq_of(c)] = bytes(c)
    r = Reconstructor(media, ssrc)
    r.set_fec_packet(fec)
    if r.refused:
        return REFUSED, None
    if r.num_missing == 0:
        return COMPLETE, None
    if not r.can_recover():
        return WAIT, None
    return r.recover()


class FECReceiver:
    """reverseTransform over lists of packets (bytes or None) that have been unprotected."""

    def __init__(self, ssrc, ulpfec_pt):
        self.ssrc, self.ulpfec_pt = ssrc, ulpfec_pt & 0x7F
        self.nb_fec = self.nb_recovered = 0
        self.media, self.fecs = {}, {}
        self.reconstructor = Reconstructor(self.media, ssrc)

    def save_fec(self, p):  # :350-356
        if len(self.fecs) >= FEC_BUF_SIZE:
            del self.fecs[first_key(self.fecs)]
        self.fecs[seq_of(p)] = bytes(p)

    def save_media(self, p):  # :364-389
        if len(self.media) >= MEDIA_BUF_SIZE:
            del self.media[first_key(self.media)]
        self.media[seq_of(p)] = bytes(p)

    def reverse_transform(self, pkts):  # :233-319
        pkts = list(pkts)
        for i, pkt in enumerate(pkts):
            if pkt is None:
                continue
            if (pkt[1] & 0x7F) == self.ulpfec_pt:
                self.nb_fec += 1
                pkts[i] = None
                self.save_fec(pkt)
            else:
                self.save_media(pkt)
        to_remove = []
        for key in sorted(self.fecs, key=functools.cmp_to_key(seq_cmp)):
            fec = self.fecs[key]
            self.reconstructor.set_fec_packet(fec)
            if self.reconstructor.refused:
                continue  # the defined deviation: the packet stays and is asked again
            if self.reconstructor.num_missing == 0:
                to_remove.append(key)
                continue
            if self.reconstructor.can_recover():
                to_remove.append(key)
                code, recovered = self.reconstructor.recover()
                if code == REFUSED:
                    to_remove.pop()
                if recovered is not None:
                    self.nb_recovered += 1
                    self.save_media(recovered)
                    if None in pkts:
                        pkts[pkts.index(None)] = recovered
                    else:
                        pkts.append(recovered)
        for key in to_remove:
            self.fecs.pop(key, None)
        return pkts
