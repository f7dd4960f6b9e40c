"""The GPU AES-GCM entry point as seen without a GPU: the symbol is exported
and declared, refuses a NULL engine before it touches the device, and the
Python mirror exists.  Its key block is checked against the host AEAD's own
table and key schedule by tools/gcm_host_check.cpp."""
import ctypes

from libjitsi_amd import _native as N
from libjitsi_amd import srtp


def test_symbol_is_exported_and_declared():
    assert "srtp_aes_gcm_device" in N.EXPORTED
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "srtp_aes_gcm_device")
    assert "int srtp_aes_gcm_device(srtp_engine *e, int32_t open," in open(N.HEADER_PATH).read()


def test_null_engine_is_einval_without_a_device():
    """No engine, no launch: SRTP_EINVAL on a host with or without a GPU
    (srtp_device_count() may be 0 here; loading the library must not need one)."""
    L = N.lib()
    assert L.srtp_device_count() >= 0
    for n in (0, 1):
        assert L.srtp_aes_gcm_device(None, 0, bytes(16), 16, None, None, None, None, None, None, None, n,
                                     None) == -1


def test_python_mirror_exists():
    import inspect
    sig = inspect.signature(srtp.aes_gcm_device)
    assert list(sig.parameters)[:8] == ["engine", "key", "seg", "off", "aad_len", "length", "iv", "tag"]
    assert sig.parameters["open"].default is False and sig.parameters["result"].default is None
