"""GPU: every cipher route against the oracle over the packet-shape grids of
tests/shapes.py (header shapes that start the payload at 0, 4, 8 and 12 mod 16,
every payload and MAC-input residue, SRTCP of lengths that are no multiple of
4, headers longer than the packet or negative).  The other parity tests build
their packets with libjitsi_amd/synth.py: 12- or 20-byte headers, random
lengths, SRTCP rounded to whole words.

Each case is harness.Twin.run -- statuses, lengths, the whole segment (the
random bytes behind each packet included) and the touched contexts' state, bit
for bit against oracle/srtp_oracle.c, whose answers on these grids
test_packet_shapes_host.py holds to oracle/pyref.py -- over protect,
shapes.tamper, unprotect, and the same unprotect again (all replays).

The routes are chosen with the engine's debug hooks and bundle sizes:

  small            no hook, slices of at most 255 packets      k_small
  fused_ctr_small  DEBUG_NO_SMALL, the whole grid in a bundle  k_protect / k_unprotect + k_ctr_small
  split            DEBUG_FORCE_WIDE, the whole grid            k_ctr_wide + k_mac_wide
  fused_big        DEBUG_NO_WIDE, 8880 packets and more        the fused kernels alone (small_ctr == 0)

That a hook and a size lead to that route is plan_bundle's contract
(libjitsi_amd/csrc/bundle_plan.h), swept on the host by tools/bundle_plan_check
and test_bundle_plan_host.py; the cases here confirm only what the engine
already reports: stats()["small_bundles"] rises by one per bundle on `small`
and stands still on the others.  Engines that hold an F8, Twofish or Skein key
set have the fused kernels only (k_ext, k_skein with them), and take them at
both sizes without a hook; so does one with an AES-256-CM key set (k_ext).  The AES-GCM cases hold the wave, lane, one-pass and
one-launch routes to tests/gcm_ref.py, computed once per key size.
"""
import functools

import numpy as np
import pytest

import gcm_ref as G
import shapes
import test_gcm_engine as E
from harness import Twin
from libjitsi_amd import profile_policies, synth
from libjitsi_amd import _native as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x5A9E
SMALL_MAX = 255  # bundle_plan.h kSmallMaxN
BIG_REPS = 10    # 8880 packets: above bundle_plan.h kSmallCtrMax (8192)
WIDE_PROFILES = ("AES_CM_128_HMAC_SHA1_80", "AES_CM_128_HMAC_SHA1_32", "NULL_HMAC_SHA1_80")
# k_ext / k_skein key sets (engine.cpp: a 32-byte AES-CM key is k_ext's too, so an
# engine that holds one has neither k_small nor the split path)
FUSED_PROFILES = ("AES_256_CM_HMAC_SHA1_80", "F8_128_HMAC_SHA1_80", "TWOFISH_CM_128_HMAC_SHA1_80",
                  "TWOFISH_F8_128_HMAC_SHA1_80", "AES_CM_128_SKEIN_64")
ROUTES = {"small": 0, "fused_ctr_small": N.DEBUG_NO_SMALL, "split": N.DEBUG_FORCE_WIDE,
          "fused_big": N.DEBUG_NO_WIDE}
OK, DROP_REPLAY, DROP_AUTH, DROP_INVALID = N.STATUS_OK, 1, 2, 7


@functools.lru_cache(maxsize=None)
def _grid(name):
    return {"rtp": lambda: shapes.rtp_grid(SEED), "rtp_big": lambda: shapes.rtp_grid(SEED, reps=BIG_REPS),
            "rtcp": lambda: shapes.rtcp_grid(SEED), "quirk": lambda: shapes.quirk_grid(SEED)}[name]()


def grid(name):
    return _grid(name).copy()


def small_count(e):
    return e.stats()["small_bundles"]


def new_engine(engine_factory, **kw):
    return engine_factory(max_contexts=1 << 12, max_factories=1 << 10, max_transformers=1 << 10, **kw)


_key_seed = [9000]


class Streams:
    """A sender and a receiver transformer of each kind for one profile."""

    def __init__(self, twin, profile):
        _key_seed[0] += 1
        pols = profile_policies(profile)
        (k, s), (k2, _) = synth.keys(_key_seed[0], 2)
        k = k + k2 if pols[0].encKeyLength == 32 else k  # a 32-byte master key for AES-256
        self.facs = [twin.factory(True, k, s, *pols), twin.factory(False, k, s, *pols)]
        self.snd = {kind: twin.transformer(kind, self.facs[0]) for kind in (O.KIND_RTP, O.KIND_RTCP)}
        self.rcv = {kind: twin.transformer(kind, self.facs[1]) for kind in (O.KIND_RTP, O.KIND_RTCP)}

    def close(self):
        for t in list(self.snd.values()) + list(self.rcv.values()):
            t.close()


def per_packet(s, kinds, side):
    """One transformer per packet: s's `side` ("snd" / "rcv") one of its kind."""
    return [getattr(s, side)[k] for k in kinds]


def run_case(twin, b, snd, rcv, abort=True, size=None, state_rows=None, restores=True):
    """Protect b, tamper, unprotect, unprotect again, each pass in bundles of
    up to `size` packets (None: one bundle).  snd / rcv: a TwinTransformer or a
    list with one per packet.  state_rows: check the contexts of these packets
    only (a large bundle).  restores: an accepted packet comes back as it was
    sent (not so where the header walk ciphers header bytes).  Returns the three status arrays and the number of
    bundles per pass."""
    n = b.n
    cuts = [(a, min(a + (size or n), n)) for a in range(0, n, size or n)]

    def one_pass(cur, ts, reverse):
        parts = shapes.slices(cur, size or n)
        outs, sts = [], []
        for (a, z), sub in zip(cuts, parts):
            t = ts[a:z] if isinstance(ts, list) else ts
            seg, ln, st = twin.run(t, reverse, sub.seg, sub.off, sub.length, sub.cap, abort_on_error=abort,
                                   check_state=state_rows is None)
            if state_rows is not None:
                rows = [i - a for i in state_rows if a <= i < z]
                per = t if isinstance(t, list) else [t] * sub.n
                twin.check_states([per[i] for i in rows], sub.seg, sub.off[rows], sub.length[rows])
            o = sub.copy()
            o.seg, o.length = seg, ln
            outs.append(o)
            sts.append(st)
        return synth.concat(outs), np.concatenate(sts)

    pb, st1 = one_pass(b, snd, False)
    tb = shapes.tamper(pb, pb.length)
    ub, st2 = one_pass(tb, rcv, True)
    _, st3 = one_pass(tb, rcv, True)
    for i in np.nonzero(st2 == OK)[0][::7] if restores else ():
        assert ub.length[i] == b.length[i] and ub.packet(i) == b.packet(i)
    return st1, st2, st3, len(cuts)


def check_counts(name, profile, st1, st2, st3):
    """The counts test_packet_shapes_host.py pins for the two references; and
    SRTP's second unprotect accepts nothing (the reference's SRTCP window moves
    backwards with an older index, so there some replays pass: left to the
    oracle)."""
    n1, n2 = np.bincount(st1, minlength=10), np.bincount(st2, minlength=10)
    if name == "rtp":
        # every tampered packet refused, every other accepted (refused by the tag check;
        # a few of the 8880 have their SSRC turned into a later repetition's: replays there)
        assert n1[OK] == len(st1) and (st2[::3] != OK).all() and n2[OK] * 3 == 2 * len(st2)
        assert n2[OK] + n2[DROP_AUTH] + n2[DROP_REPLAY] == len(st2)
        assert not (st3 == OK).any()
    elif name == "rtcp":
        assert n1[OK] == 132 and n1[DROP_INVALID] == 4
        if not profile.startswith("NULL"):  # (a NULL-cipher sender repeats index 0: replays)
            assert n2[OK] == 88 and n2[DROP_AUTH] == 44 and n2[DROP_INVALID] == 4


def rtp_and_rtcp_big():
    """rtp_grid x 10 with rtcp_grid behind it, and each packet's kind."""
    big, rtcp = grid("rtp_big"), grid("rtcp")
    return synth.concat([big, rtcp]), [O.KIND_RTP] * big.n + [O.KIND_RTCP] * rtcp.n


def big_state_rows(n_rtp, n):
    """The first repetition's packets (its 11 SSRCs) and the SRTCP tail."""
    return list(range(shapes.RTP_N)) + list(range(n_rtp, n))


# ------------------------------------ 1. engines with the split path's key sets
@pytest.fixture(scope="module")
def wide(engine_factory, oracle):
    """wide(abort): the module's engine with abort-on-throw on or off; it only
    ever holds key sets of WIDE_PROFILES."""
    made = {}

    def get(abort):
        if abort not in made:
            made[abort] = Twin(new_engine(engine_factory, abort_on_error=abort))
        return made[abort]

    return get


WIDE_CELLS = [(r, g) for r in ("small", "fused_ctr_small", "split") for g in ("rtp", "rtcp")]
WIDE_CELLS.append(("fused_big", "rtp+rtcp"))


@pytest.mark.parametrize("profile", WIDE_PROFILES)
@pytest.mark.parametrize("route,name", WIDE_CELLS, ids=["%s-%s" % c for c in WIDE_CELLS])
def test_wide_engine_routes(wide, route, name, profile):
    """rtp_grid and rtcp_grid on the four routes of an engine whose key sets
    are all AES-CM / NULL cipher + HMAC-SHA1."""
    twin = wide(True)
    eng = twin.engine
    s = Streams(twin, profile)
    eng.set_debug(ROUTES[route])
    try:
        c0 = small_count(eng)
        if route == "fused_big":
            b, kinds = rtp_and_rtcp_big()
            st1, st2, st3, nb = run_case(twin, b, per_packet(s, kinds, "snd"), per_packet(s, kinds, "rcv"),
                                       state_rows=big_state_rows(BIG_REPS * shapes.RTP_N, b.n))
            check_counts("rtp", profile, st1[:-136], st2[:-136], st3[:-136])
            check_counts("rtcp", profile, st1[-136:], st2[-136:], st3[-136:])
        else:
            kind = O.KIND_RTP if name == "rtp" else O.KIND_RTCP
            st1, st2, st3, nb = run_case(twin, grid(name), s.snd[kind], s.rcv[kind],
                                       size=SMALL_MAX if route == "small" else None)
            check_counts(name, profile, st1, st2, st3)
        assert small_count(eng) - c0 == (3 * nb if route == "small" else 0)
    finally:
        eng.set_debug(0)
        s.close()


@pytest.mark.parametrize("profile", WIDE_PROFILES)
@pytest.mark.parametrize("route", ["small", "fused_ctr_small", "split"])
@pytest.mark.parametrize("abort", [True, False], ids=["abort", "each"])
def test_wide_engine_quirks(wide, abort, route, profile):
    """quirk_grid on the three routes a bundle of 144 packets can take, with
    abort-on-throw (the first packet throws, the rest is not processed) and
    without (each packet on its own: rtp_header_len's signed extension length,
    ctr_would_throw's negative payload lengths)."""
    twin = wide(abort)
    eng = twin.engine
    s = Streams(twin, profile)
    eng.set_debug(ROUTES[route])
    try:
        c0 = small_count(eng)
        st1, st2, st3, nb = run_case(twin, grid("quirk"), s.snd[O.KIND_RTP], s.rcv[O.KIND_RTP], abort=abort,
                                     restores=False)
        assert small_count(eng) - c0 == (3 if route == "small" else 0)
        if profile.startswith("AES"):
            n1 = np.bincount(st1, minlength=10)
            assert (n1[6], n1[8]) == ((1, 143) if abort else (82, 0))
    finally:
        eng.set_debug(0)
        s.close()


# --------------------------------- 2. engines that have the fused kernels only
@pytest.fixture(scope="module", params=FUSED_PROFILES)
def fused(request, engine_factory, oracle):
    t = Twin(new_engine(engine_factory))
    t.profile = request.param
    return t


@pytest.mark.parametrize("name", ["rtp", "rtcp", "rtp+rtcp_big"])
def test_fused_only_engines(fused, name):
    """AES-256-CM, F8, Twofish-CM, Twofish-F8 (k_ext) and AES-CM + Skein-MAC
    (k_skein): the whole grid in one bundle (with k_ctr_small where the cipher
    is AES-128-CM), and 8880 packets and more (without)."""
    eng = fused.engine
    s = Streams(fused, fused.profile)
    try:
        c0 = small_count(eng)
        if name == "rtp+rtcp_big":
            b, kinds = rtp_and_rtcp_big()
            st1, st2, st3, _ = run_case(fused, b, per_packet(s, kinds, "snd"), per_packet(s, kinds, "rcv"),
                                      state_rows=big_state_rows(BIG_REPS * shapes.RTP_N, b.n))
            check_counts("rtp", fused.profile, st1[:-136], st2[:-136], st3[:-136])
            check_counts("rtcp", fused.profile, st1[-136:], st2[-136:], st3[-136:])
        else:
            kind = O.KIND_RTP if name == "rtp" else O.KIND_RTCP
            st1, st2, st3, _ = run_case(fused, grid(name), s.snd[kind], s.rcv[kind])
            check_counts(name, fused.profile, st1, st2, st3)
        assert small_count(eng) == c0
    finally:
        s.close()


@pytest.mark.parametrize("profile", ["AES_256_CM_HMAC_SHA1_80", "F8_128_HMAC_SHA1_80", "AES_CM_128_SKEIN_64"])
def test_fused_only_quirks(engine_factory, oracle, profile):
    """quirk_grid, each packet on its own, through k_ext (AES-256-CM's and F8's
    own rules for what throws) and k_skein."""
    twin = Twin(new_engine(engine_factory, abort_on_error=False))
    s = Streams(twin, profile)
    st1, _, _, _ = run_case(twin, grid("quirk"), s.snd[O.KIND_RTP], s.rcv[O.KIND_RTP], abort=False, restores=False)
    assert np.bincount(st1, minlength=10)[6] == (36 if profile.startswith("F8") else 82)
    assert small_count(twin.engine) == 0


# ------------------------------------------------------- 3. one mixed bundle
def test_mixed_profiles_one_bundle(engine_factory, oracle):
    """All eight profiles above in one engine, an SRTP and an SRTCP transformer
    each; rtp_grid + rtcp_grid with packet i on transformer i % 8 of its kind
    (each with its own SSRCs), so every wave mixes key sets, MACs and header
    shapes."""
    twin = Twin(new_engine(engine_factory))
    streams = [Streams(twin, p) for p in WIDE_PROFILES + FUSED_PROFILES]
    rtp = shapes.spread_ssrcs(grid("rtp"), False, len(streams))
    rtcp = shapes.spread_ssrcs(grid("rtcp"), True, len(streams))
    b = synth.concat([rtp, rtcp])
    kinds = [O.KIND_RTP] * rtp.n + [O.KIND_RTCP] * rtcp.n
    who = list(range(rtp.n)) + list(range(rtcp.n))  # i % 8 within each kind
    snd = [streams[w % 8].snd[k] for w, k in zip(who, kinds)]
    rcv = [streams[w % 8].rcv[k] for w, k in zip(who, kinds)]
    st1, st2, st3, _ = run_case(twin, b, snd, rcv)
    check_counts("rtp", "", st1[:rtp.n], st2[:rtp.n], st3[:rtp.n])
    assert (st1[rtp.n:] == OK).sum() == 132
    assert small_count(twin.engine) == 0


# ------------------------------------------------------------- 4. AES-GCM
GCM_PAYLOADS = tuple(range(34)) + (47, 48, 49, 1188)
GCM_ROUTES = {
    "wave": 0,
    "lane": N.DEBUG_NO_GCM_WAVE,
    "wave_one_pass": N.DEBUG_FORCE_GCM_SPEC,
    "lane_one_pass": N.DEBUG_NO_GCM_WAVE | N.DEBUG_FORCE_GCM_SPEC,
    "small": N.DEBUG_FORCE_SMALL,
}
GCM_PROFILES = {"AEAD_AES_128_GCM": E.GCM128, "AEAD_AES_256_GCM": E.GCM256}


def gcm_grid():
    """The 12 header shapes x GCM_PAYLOADS, SSRCs and sequences as rtp_grid's,
    in 16-byte aligned regions with 20 bytes of room and random bytes behind
    each packet."""
    rng = np.random.default_rng(SEED + 1)
    pk = []
    for cc, ext in shapes.HEADER_SHAPES:
        for plen in GCM_PAYLOADS:
            i = len(pk)
            pk.append(G.rtp_packet(0x4000 + i % 11, (65500 + i // 11) & 0xFFFF,
                                   rng.integers(0, 256, plen, dtype=np.uint8).tobytes(), csrcs=cc, ext_words=ext))
    seg, off, ln, cap = G.pack(pk, room=20)
    fill = rng.integers(0, 256, len(seg), dtype=np.uint8)
    for i, p in enumerate(pk):
        a = int(off[i]) + len(p)
        z = int(off[i + 1]) if i + 1 < len(pk) else len(seg)
        seg[a:z] = fill[a:z]
    return seg, off, ln, cap


@functools.lru_cache(maxsize=None)
def gcm_expected(profile):
    """gcm_ref's protect, tamper, unprotect and second unprotect of gcm_grid(),
    and its contexts afterwards: computed once, shared by the routes."""
    pol = GCM_PROFILES[profile]
    mk, ms = E.keys(700 + pol[1], pol[1])
    f = G.Factory(True, mk, ms, pol, pol)
    snd, rcv = G.Transformer(0, f, f), G.Transformer(0, f, f)
    seg0, off, ln0, cap = gcm_grid()
    seg1, ln1 = seg0.copy(), ln0.copy()
    st1 = G.process(snd, False, seg1, off, ln1, cap)
    tin = shapes.tamper_seg(seg1, off, ln1)
    seg2, ln2 = tin.copy(), ln1.copy()
    st2 = G.process(rcv, True, seg2, off, ln2, cap)
    seg3, ln3 = tin.copy(), ln1.copy()
    st3 = G.process(rcv, True, seg3, off, ln3, cap)
    # (input bytes, input lengths, expected bytes, lengths, statuses) per pass
    steps = [(seg0, ln0, seg1, ln1, st1), (tin, ln1, seg2, ln2, st2), (tin, ln1, seg3, ln3, st3)]
    states = {"snd": {s: snd.state(s) for s in snd.ctx}, "rcv": {s: rcv.state(s) for s in rcv.ctx}}
    return (mk, ms, pol, off, cap), steps, states


@pytest.fixture(scope="module")
def gcm_engine(engine_factory):
    e = new_engine(engine_factory)
    e.enable_aead()
    return e


@pytest.mark.parametrize("profile", list(GCM_PROFILES))
@pytest.mark.parametrize("route", list(GCM_ROUTES))
def test_gcm_routes(gcm_engine, route, profile):
    """The header shapes x payloads 0..33, 47..49, 1188 under AES-GCM, on the
    wave and lane kernels, each with the two-pass and the one-pass open, and on
    k_small's GCM instance (slices of at most 255 packets); statuses, lengths,
    the whole segment and the exported contexts against gcm_ref."""
    e = gcm_engine
    (mk, ms, pol, off, cap), steps, states = gcm_expected(profile)
    n = len(off)
    assert np.bincount(steps[0][4], minlength=3).tolist()[:3] == [n, 0, 0]
    assert np.bincount(steps[1][4], minlength=3).tolist()[:3] == [n - n // 3, 0, n // 3]
    assert (steps[2][4] != OK).all()
    f = E.F(e, True, mk, ms, pol)
    snd, rcv = E.T(E.RTP, f), E.T(E.RTP, f)
    size = SMALL_MAX if route == "small" else n
    e.set_debug(GCM_ROUTES[route])
    try:
        c0 = e.stats()
        for (seg_in, ln_in, seg_x, ln_x, st_x), t, reverse in zip(steps, (snd, rcv, rcv), (False, True, True)):
            for a in range(0, n, size):
                z = min(a + size, n)
                lo, hi = int(off[a]), (int(off[z]) if z < n else len(seg_in))
                seg, ln = seg_in[lo:hi].copy(), ln_in[a:z].copy()
                st = e.transform_host(reverse, t.tid, seg, (off[a:z] - off[a]).astype(np.uint32), ln, cap[a:z])
                assert st.tolist() == st_x[a:z].tolist(), (reverse, a)
                assert ln.tolist() == ln_x[a:z].tolist(), (reverse, a)
                if not np.array_equal(seg, seg_x[lo:hi]):
                    d = np.nonzero(seg != seg_x[lo:hi])[0] + lo
                    pkt = np.searchsorted(off.astype(np.int64), d[:4], side="right") - 1
                    raise AssertionError(f"segment differs at {d[:4].tolist()} (packets {pkt.tolist()}, len in "
                                         f"{ln_in[pkt].tolist()}, reverse={reverse}); {len(d)} bytes")
        c1 = e.stats()
        bundles = 3 * ((n + size - 1) // size)
        assert c1["small_aead_bundles"] - c0["small_aead_bundles"] == (bundles if route == "small" else 0)
        assert c1["small_bundles"] == c0["small_bundles"]
        for side, t in (("snd", snd), ("rcv", rcv)):
            got = e.export_contexts(t.e)
            assert sorted(got) == sorted(states[side])
            for ssrc, want in states[side].items():
                for k in E.KEYS_RTP:
                    assert int(got[ssrc][k]) == int(want[k]), (side, hex(ssrc), k, want, got[ssrc])
    finally:
        e.set_debug(0)
        snd.e.close()
        rcv.e.close()
