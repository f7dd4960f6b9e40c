"""CPU: srtp_stats grew by one counter at its end, small_aead_bundles (bundles
run by k_small's GCM instance), and the Python mirror follows the header."""
import ctypes as C
import os
import re

from libjitsi_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srtp_mi355x.h")
BEFORE = ("bundles", "packets", "status", "roc_rechecks", "repaired", "ctx_overflow", "ctx_live", "ctx_tombstones",
          "ctx_slots", "rehashes", "chain_stalls", "long_walked", "holes", "small_bundles")


def test_stats_ends_with_small_aead_bundles():
    names = [n for n, _ in N.Stats._fields_]
    assert tuple(names[:-1]) == BEFORE
    assert names[-1] == "small_aead_bundles"
    assert N.Stats.small_aead_bundles.offset == C.sizeof(N.Stats) - 8


def test_stats_is_eight_bytes_larger():
    before = 8 * (len(BEFORE) - 1) + 8 * N.NUM_STATUS  # every field a uint64_t, status[] NUM_STATUS of them
    assert C.sizeof(N.Stats) == before + 8
    assert "small_aead_bundles" in N.Stats().as_dict()


def test_header_agrees():
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_stats;", text).group(1)
    fields = [m.group(1) for decl in re.findall(r"uint64_t([^;]*);", body)
              for m in re.finditer(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in N.Stats._fields_]
