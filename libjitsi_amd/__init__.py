"""libjitsi_amd -- MI355X-native SRTP/SRTCP packet-crypto engine.

A drop-in for the per-packet hot path of libjitsi's SRTPTransformer /
SRTCPTransformer (AES_CM_128_HMAC_SHA1_80/_32, F8_128_HMAC_SHA1_80 and NULL-cipher
profiles):
bundles of packets from many SSRC contexts are protected/unprotected by
hand-written gfx950 kernels behind the C ABI in include/srtp_mi355x.h.
"""
from .srtp import (PacketTransformer, RawPacket, SRTCPTransformer, SRTPAggregator,  # noqa: F401
                   SRTPContextFactory, SRTPDispatcher,
                   SRTPEngine, SRTPPipeline, SRTPPolicy, SRTPTransformer, SRTPTransformException, pack,
                   HostBuffer, host_is_registered, host_register, host_unregister, profile_policies, transform_bundle,
                   fan_out, fan_out_rw, fan_out_ast, abs_send_time, fan_out_pay, fec_sn_bytes, reverse_transform_levels,
                   fan_out_red, RED_OFF, RED_STRIP, RED_WRAP, fan_out_fec, FecSender, FecReceiver)
from . import _native  # noqa: F401

__all__ = ["PacketTransformer", "RawPacket", "SRTCPTransformer", "SRTPAggregator", "SRTPContextFactory", "SRTPDispatcher", "SRTPEngine",
           "SRTPPipeline", "SRTPPolicy", "SRTPTransformer", "SRTPTransformException", "pack", "profile_policies",
           "transform_bundle", "fan_out", "fan_out_rw", "fan_out_ast", "abs_send_time", "fan_out_pay", "fan_out_red", "fan_out_fec", "FecSender", "FecReceiver", "RED_OFF", "RED_STRIP", "RED_WRAP", "fec_sn_bytes", "reverse_transform_levels", "host_register", "host_unregister", "host_is_registered", "HostBuffer"]
