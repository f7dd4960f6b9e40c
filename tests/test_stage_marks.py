"""GPU: the engine launches what the bundle's plan says (bundle_plan.h), seen
through the per-stage timing marks: one mark per run of launches of one stage.
A plain AES_CM_128_HMAC_SHA1_80 engine with timing on, one bundle per
direction at each of the three paths' sizes (k_small, the fused kernels, the
split path); every bundle's result is the oracle's bit for bit."""
import numpy as np
import pytest

from libjitsi_amd import profile_policies, synth
from libjitsi_amd import _native as N
from oracle import oracle as O

from harness import Twin

pytestmark = pytest.mark.gpu
P80 = profile_policies("AES_CM_128_HMAC_SHA1_80")


def marks(eng):
    return {stage: int(cnt) for stage, (_, cnt) in eng.read_timing().items()}


def expect(**stages):
    return {s: stages.get(s, 0) for s in N.STAGES}


@pytest.mark.parametrize("n, protect, unprotect", [
    (1, expect(protect=1), expect(verify=1)),
    (300, expect(parse=1, sort=1, walk=1, protect=1), expect(parse=1, sort=1, verify=1, walk=1, decrypt=1)),
    (2048, expect(parse=1, sort=1, walk=1, protect=1), expect(parse=1, sort=1, verify=1, walk=1, decrypt=1)),
], ids=["small_1", "fused_300", "split_2048"])
def test_marks_per_stage(engine_factory, oracle, n, protect, unprotect):
    eng = engine_factory(max_contexts=1 << 12, max_factories=16, max_transformers=16)
    twin = Twin(eng)
    (k, s), = synth.keys(7300 + n, 1)
    snd = twin.transformer(O.KIND_RTP, twin.factory(True, k, s, *P80))
    rcv = twin.transformer(O.KIND_RTP, twin.factory(False, k, s, *P80))
    b = synth.rtp_bundle(n, min(n, 16), (60, 1400), seed=7400 + n)
    eng.set_timing(True)
    small0 = eng.stats()["small_bundles"]
    marks(eng)  # whatever lay there
    seg, ln, st = twin.run(snd, False, b.seg, b.off, b.length, b.cap)
    assert marks(eng) == protect
    assert (st == N.STATUS_OK).all()
    marks(eng)
    _, _, st = twin.run(rcv, True, seg, b.off, ln, b.cap)
    assert marks(eng) == unprotect
    assert (st == N.STATUS_OK).all()
    assert eng.stats()["small_bundles"] - small0 == (2 if n == 1 else 0)
