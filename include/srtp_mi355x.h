/*
 * srtp_mi355x.h -- C ABI of the MI355X SRTP/SRTCP packet-crypto engine.
 *
 * Drop-in boundary for libjitsi's SRTP hot path.  Each entry point replaces a
 * reference Java API (paths relative to src/org/jitsi/impl/neomedia/):
 *
 *   srtp_factory_create        <- new SRTPContextFactory(sender, masterKey,
 *                                 masterSalt, srtpPolicy, srtcpPolicy)
 *                                 transform/srtp/SRTPContextFactory.java:50-68
 *   srtp_factory_close         <- SRTPContextFactory.close()          :74-86
 *   srtp_transformer_create    <- new SRTPTransformer(fwd, rev)
 *                                 transform/srtp/SRTPTransformer.java:82-90,
 *                                 new SRTCPTransformer(fwd, rev)
 *                                 transform/srtp/SRTCPTransformer.java:73-80
 *   srtp_transformer_set_factory <- SRTPTransformer.setContextFactory :100-125,
 *                                 SRTCPTransformer.updateFactory      :92-117
 *   srtp_transformer_close     <- SRTPTransformer.close() :132-150,
 *                                 SRTCPTransformer.close() :124-142
 *   srtp_transform_device /    <- PacketTransformer.transform(RawPacket[]) and
 *   srtp_transform_host           .reverseTransform(RawPacket[])
 *                                 transform/PacketTransformer.java:28-53 as
 *                                 implemented by SinglePacketTransformer
 *                                 transform/SinglePacketTransformer.java:121-216
 *                                 over SRTPTransformer.transform/reverseTransform
 *                                 transform/srtp/SRTPTransformer.java:185-219
 *                                 (per packet: SRTPCryptoContext.transformPacket
 *                                 :658-705 / reverseTransformPacket :572-642,
 *                                 SRTCPCryptoContext.transformPacket :391-427 /
 *                                 reverseTransformPacket :315-374)
 *   srtp_engine_opts.check_replay <- ConfigurationService property
 *                                 ...srtp.SRTPCryptoContext.checkReplay
 *                                 (SRTPCryptoContext.java:80-121)
 *
 * Packet bundle model (RawPacket[] -> packed segment).  Packet i occupies
 * seg[off[i] .. off[i] + cap[i]) and its current RTP/RTCP length is len[i]
 * (RawPacket.length).  The engine works in place: protect appends the tag (and
 * for SRTCP the E|index word) inside cap[i]; unprotect shrinks len[i].
 * Requirements: off[i] % 16 == 0, cap[i] <= 65535, and the segment must be
 * readable and writable up to off[i] + roundup16(cap[i]) for every packet.
 * status[i] receives one SRTP_STATUS_* value; "drop" statuses correspond to
 * the reference returning null for that element.
 *
 * Ownership: the caller owns every buffer; the engine owns contexts, session
 * keys and device scratch, and zeroes keys when factories are closed.
 * Threading: calls on one engine are serialised internally and are safe from
 * any host thread: each call makes the engine's device current for its
 * duration and restores the caller's device (one process may drive engines on
 * several GPUs).  Bundles of one engine are processed in submission order
 * (== the order the reference's `synchronized` contexts give): a bundle
 * submitted on another stream than the engine's previous bundle waits for
 * that bundle on the device, with no host stall.  Control-plane calls
 * (factory/transformer close and rekey, context state, stats) first wait for
 * every bundle the engine has enqueued.  Independent directions that should
 * overlap on the device use one engine each (e.g. a send-side and a
 * receive-side engine).
 */
#ifndef SRTP_MI355X_H
#define SRTP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRTP_MI355X_ABI_VERSION 5

/* SRTPPolicy constants (transform/srtp/SRTPPolicy.java:29-63) */
#define SRTP_NULL_ENCRYPTION 0
#define SRTP_AESCM_ENCRYPTION 1
#define SRTP_AESF8_ENCRYPTION 2 /* SRTPCipherF8 (SDES F8_128_HMAC_SHA1_80) */
#define SRTP_TWOFISH_ENCRYPTION 3   /* counter mode over Twofish (ZRTP "2FS") */
#define SRTP_TWOFISHF8_ENCRYPTION 4 /* F8 over Twofish */
/* AES-GCM, the AEAD profiles of RFC 7714 (AEAD_AES_128_GCM / AEAD_AES_256_GCM;
 * later libjitsi's SRTPPolicy.AESGCM_ENCRYPTION).  The policy shape is
 * {SRTP_AESGCM_ENCRYPTION, enc_key_len 16 or 32, SRTP_NULL_AUTHENTICATION,
 * auth_key_len 0, auth_tag_len 16, salt_key_len 12}.
 * The engine's packet path runs it behind a per-engine switch,
 * srtp_engine_enable_aead (off on a new engine: srtp_factory_create then
 * answers SRTP_EPOLICY for such a policy, as for any other GCM-typed shape
 * with the switch on).  Either policy of a factory, or both, may be GCM.
 * Packets: SRTP header as AAD, ciphertext, 16-byte tag; SRTCP header(8),
 * ciphertext, tag, E|index word, the word being AAD too (RFC 7714 8-9;
 * statuses and lengths in srtp_gcm_packet_job).  Bundles
 * (srtp_transform_*, srtp_pipeline_*, srtp_dispatch_*) and the per-packet paths
 * (srtp_aggregator_*, srtp_queue_*, srtp_rawpacket_*) alike: an aggregator or
 * RawPacket batch created after the switch was turned on leaves 20 bytes of
 * trailer room, what GCM SRTCP appends (srtp_engine_trailer_room).  Still
 * closed to GCM key sets: k_small, its direct mode and the split path.  Beside it: the key derivation of RFC 7714 11
 * (srtp_derive_session_keys_for), the AEAD on the host (srtp_aes_gcm) and as a
 * stateless GPU batch (srtp_aes_gcm_device), the dispatcher's may-throw test
 * (srtp_packet_may_throw, tag_mask bit 16), and the DTLS-SRTP ids
 * SRTP_PROFILE_AEAD_AES_*_GCM through srtp_dtls_profile_keys_ex. */
#define SRTP_AESGCM_ENCRYPTION 5
#define SRTP_NULL_AUTHENTICATION 0
#define SRTP_HMACSHA1_AUTHENTICATION 1
#define SRTP_SKEIN_AUTHENTICATION 2 /* Skein-512 MAC, tag_len * 8 output bits (ZRTP "SK32"/"SK64") */

/* transformer kinds */
#define SRTP_KIND_RTP 0  /* SRTPTransformer */
#define SRTP_KIND_RTCP 1 /* SRTCPTransformer */

/* per-packet status */
#define SRTP_STATUS_OK 0
#define SRTP_STATUS_DROP_REPLAY 1     /* checkReplay() false */
#define SRTP_STATUS_DROP_AUTH 2       /* authenticatePacket() false */
#define SRTP_STATUS_DROP_VERSION 3    /* (byte0 & 0xC0) != 0x80 (SRTPTransformer.java:189) */
#define SRTP_STATUS_DROP_NO_CONTEXT 4 /* factory closed, no context for the SSRC */
#define SRTP_STATUS_ERR_CAPACITY 5    /* cap[i] too small for the appended trailer */
#define SRTP_STATUS_ERR_MALFORMED 6   /* the reference throws on this packet */
#define SRTP_STATUS_DROP_INVALID 7    /* len < 12 or len > cap (RawPacket.isInvalid) */
#define SRTP_STATUS_NOT_PROCESSED 8   /* after an ERR_MALFORMED with abort_on_error */
#define SRTP_STATUS_SKIPPED 9         /* SRTP_PKT_FLAG_SKIP (null element / predicate) */
#define SRTP_STATUS_ERR_INTERNAL 10   /* no walk reached the packet: an engine bug (never expected);
                                         the packet and its context are left as they were */
#define SRTP_NUM_STATUS 11

/* per-packet flags (javax.media.Buffer values read at SRTPCryptoContext.java:609) */
#define SRTP_PKT_FLAG_DISCARD 0x2u
#define SRTP_PKT_FLAG_SILENCE 0x4u
#define SRTP_PKT_FLAG_SKIP 0x80000000u

/* return codes */
#define SRTP_OK 0
#define SRTP_EINVAL -1
#define SRTP_ENOMEM -2
#define SRTP_EFULL -3   /* context / factory / transformer table full */
#define SRTP_EDEVICE -4 /* HIP runtime error */
#define SRTP_EPOLICY -5 /* policy outside the implemented ciphers x MACs (see srtp_factory_create) */
#define SRTP_EAGAIN -6  /* srtp_queue_submit: the queue is full, or no slot is free while it holds
                           completed packets -- reap, then submit again */

typedef struct srtp_engine srtp_engine;

/* SRTPPolicy(encType, encKeyLength, authType, authKeyLength, authTagLength,
 * saltKeyLength) -- SRTPPolicy.java:107-120 */
typedef struct {
    int32_t enc_type, enc_key_len, auth_type, auth_key_len, auth_tag_len, salt_key_len;
} srtp_policy;

typedef struct {
    int32_t device;            /* HIP device ordinal */
    int32_t check_replay;      /* SRTPCryptoContext.checkReplay, default 1 */
    int32_t abort_on_error;    /* SinglePacketTransformer rethrow semantics, default 1 */
    uint32_t max_contexts;     /* (transformer, SSRC) contexts, default 1<<20 (table of
                                  next_pow2(2 * max_contexts) slots, 40 B each) */
    uint32_t max_factories;    /* default 1<<16 */
    uint32_t max_transformers; /* default 1<<16 */
    uint32_t max_batch;        /* initial scratch size in packets (grows), default 1<<16 */
} srtp_engine_opts;

typedef struct {
    int32_t roc, s_l, seq_num_set, guessed_roc; /* SRTP context */
    int32_t sent_index, received_index;         /* SRTCP context */
    uint64_t replay_window;
    uint32_t key_set;                           /* internal session-key slot */
} srtp_ctx_state;

int srtp_engine_opts_default(srtp_engine_opts *opts);
int srtp_engine_create(const srtp_engine_opts *opts, srtp_engine **out);
void srtp_engine_destroy(srtp_engine *e);
/* the options the engine was created with */
int srtp_engine_get_opts(srtp_engine *e, srtp_engine_opts *out);
const char *srtp_engine_last_error(srtp_engine *e);

int srtp_factory_create(srtp_engine *e, int32_t sender, const uint8_t *master_key,
                        int32_t key_len, const uint8_t *master_salt, int32_t salt_len,
                        const srtp_policy *srtp, const srtp_policy *srtcp, int32_t *out_factory);
int srtp_factory_close(srtp_engine *e, int32_t factory);

int srtp_transformer_create(srtp_engine *e, int32_t kind, int32_t fwd_factory,
                            int32_t rev_factory, int32_t *out_transformer);
int srtp_transformer_set_factory(srtp_engine *e, int32_t transformer, int32_t factory,
                                 int32_t forward);
int srtp_transformer_close(srtp_engine *e, int32_t transformer);
/* The transformer's kind and its forward factory's SRTCP policy tag length
 * (what RawPacket.grow sizes an SRTCP packet with, SRTCPCryptoContext.java:413). */
int srtp_transformer_info(srtp_engine *e, int32_t transformer, int32_t *kind,
                          int32_t *fwd_rtcp_tag_len);

/* Process one bundle whose buffers are device (HBM) pointers on the engine's
 * device; asynchronous on `stream` (a hipStream_t of that device; NULL = its
 * default stream, ordered with the caller's default-stream work).  For a
 * send-side and a receive-side engine to overlap on the device, pass each its
 * own stream (srtp_engine_stream).  tids == NULL means every
 * packet belongs to `tid`; otherwise tids[i] (device array) names packet i's
 * transformer.  flags may be NULL.  reverse = 0: transform (protect),
 * reverse = 1: reverseTransform (unprotect).  The caller guarantees what
 * srtp_transform_host checks on the host: every packet region [off[i],
 * off[i] + cap[i] rounded up to 16) lies inside the segment, off[i] is 16-byte
 * aligned and cap[i] <= 65535 (the device arrays are not read back to check). */
int srtp_transform_device(srtp_engine *e, int32_t reverse, const int32_t *tids, int32_t tid,
                          uint8_t *seg, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                          const uint32_t *flags, int32_t *status, uint32_t n, void *stream);

/* Same with host buffers: copies to HBM, runs, copies back, synchronises.
 * seg_bytes is the size of the host segment. */
int srtp_transform_host(srtp_engine *e, int32_t reverse, const int32_t *tids, int32_t tid,
                        uint8_t *seg, size_t seg_bytes, const uint32_t *off, uint32_t *len,
                        const uint32_t *cap, const uint32_t *flags, int32_t *status, uint32_t n);

/* Receive with the ssrc-audio-level read on the device.  In the reference's
 * receive chain SsrcTransformEngine stands in front of SRTP
 * (MediaStreamImpl.java:1037-1044; SsrcTransformEngine.reverseTransform,
 * SsrcTransformEngine.java:226-274): it reads the negotiated ssrc-audio-level
 * header extension (RFC 6464, RawPacket.extractSsrcAudioLevel), gives a packet
 * whose level is 127 -- a muted source -- Buffer.FLAG_SILENCE, so that it is
 * authenticated but not deciphered (SRTPCryptoContext.java:609), and hands
 * every level to the stream's audio-level dispatcher.  These entries are
 * srtp_transform_device(reverse = 1) / srtp_transform_host(reverse = 1) with
 * that stage in front (k_audio_level): entry i's level is written to level[i]
 * -- 0..127, or -128 (Byte.MIN_VALUE) where the packet carries none -- and the
 * chain then runs with flags[i] | SRTP_PKT_FLAG_SILENCE where level[i] is 127
 * and flags[i] otherwise, exactly as if the caller had made those flags on the
 * host: every route, per-context order, abort-on-throw and the counters are
 * that call's.  The level is reported whatever the packet's SRTP status turns
 * out to be; the reference, too, dispatches it before authentication.
 *
 * ext_ids == NULL: every entry uses `ext_id`; otherwise ext_ids[i] (n bytes)
 * is entry i's ID.  An entry is read only if it is not flagged
 * SRTP_PKT_FLAG_SKIP, its ID is in 1..127 (the reference tests a Java byte for
 * > 0: 0 and 128..255 are off) and 12 <= len[i] <= cap[i]
 * (!RawPacket.isInvalid); its first byte must then say version 2.  The walk is
 * the reference's, Java's signed bytes included (libjitsi_amd/csrc/
 * audio_level_job.h states it line by line), with two defined deviations where
 * the reference has no defined answer, both answering "no level": a read at or
 * past len[i] (the reference reads stale buffer bytes or throws), and a
 * two-byte-form element that is not the match and whose length byte is >= 0x80
 * (the reference's offset walks backwards).  The rule knows nothing of a
 * transformer's kind: the reference's engine has no RTCP transformer, so for
 * SRTCP entries pass ID 0.  With ext_ids NULL and ext_id 0 the call is
 * srtp_transform_device(reverse = 1) with the caller's flags, and level is
 * filled with -128.  Left to the host: dropMutedAudioSourceInReverseTransform
 * (a per-stream run counter), CSRC level lists, and the dispatcher itself.
 *
 * srtp_transform_device_lvl: device pointers, asynchronous on `stream`, the
 * caller's guarantees as for srtp_transform_device; ext_ids and level are
 * device arrays of n bytes.  srtp_transform_host_lvl: host pointers; ext_ids
 * is staged like the other small arrays and level copied back. */
int srtp_transform_device_lvl(srtp_engine *e, const int32_t *tids, int32_t tid, uint8_t *seg,
                              const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                              const uint8_t *ext_ids, uint8_t ext_id, int8_t *level, int32_t *status,
                              uint32_t n, void *stream);
int srtp_transform_host_lvl(srtp_engine *e, const int32_t *tids, int32_t tid, uint8_t *seg, size_t seg_bytes,
                            const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                            const uint8_t *ext_ids, uint8_t ext_id, int8_t *level, int32_t *status, uint32_t n);
/* Cumulative since engine creation: _lvl calls that were enqueued, the entries
 * whose bytes were read, the levels found (0..127) and the entries flagged
 * SRTP_PKT_FLAG_SILENCE (level 127). */
typedef struct {
    uint64_t calls, entries_read, levels_found, silent;
} srtp_audio_level_stats;
int srtp_engine_audio_level_stats(srtp_engine *e, srtp_audio_level_stats *out);
/* The rule of one entry (host only; audio_level_job.h, the text k_audio_level
 * compiles) over the caller's bytes: pkt holds min(len, 65535) bytes whenever
 * the entry is read (above); *level and *flags_out as the device call makes
 * them. */
int srtp_audio_level_job(const uint8_t *pkt, int32_t len, int32_t cap, uint32_t flags, uint8_t ext_id,
                         int8_t *level, uint32_t *flags_out);

/* Fan-out: one packet to many peers, expanded on the device.  A bridge receives
 * a packet once and sends it to N peers, each under its own keys -- the
 * reference's OutputDataStreamImpl.doWrite hands the same buf, off, len to every
 * stream (rtp/translator/OutputDataStreamImpl.java:171-243), and each stream's
 * connector copies it and runs its own SRTPTransformer.transform.  Here m
 * source packets (a bundle's layout: src_seg, src_off, src_len, src_cap) and n
 * destination entries, entry j = (src_idx[j], tids[j] or tid, region off[j] /
 * cap[j] of seg): entry j becomes a copy of source src_idx[j] (k_fanout, in
 * device memory) and the n entries are then protected as one bundle -- exactly
 * as if each had been a host-made copy of its source submitted in that order
 * to srtp_transform_device(reverse = 0): every profile, per-context order
 * within the bundle, abort-on-throw and the counters are that call's.  len is
 * output only.
 *
 * An entry is skipped -- nothing copied, its region untouched, len[j] = 0,
 * status SRTP_STATUS_SKIPPED -- when src_idx[j] is not in [0, m), when
 * src_status[src_idx[j]] is not SRTP_STATUS_OK (the reference's null element: a
 * packet reverseTransform dropped is never written by the translator;
 * src_status NULL: every source is OK) or when flags[j] carries
 * SRTP_PKT_FLAG_SKIP.  Otherwise len[j] = src_len[src_idx[j]] and
 * min(src_len, src_cap, cap[j]) bytes rounded up to 16 are copied; a source
 * longer than cap[j] ends SRTP_STATUS_DROP_INVALID, a region too small for the
 * trailer SRTP_STATUS_ERR_CAPACITY, by the existing rules (srtp_fanout_job is
 * the rule, on the host).  These two entries copy the source byte for byte, as
 * doWrite does; a bridge whose per-peer send chain rewrites the SSRC, sequence
 * number, timestamp or payload type in front of SRTP (simulcast, last-N) uses
 * srtp_fanout_device_rw / srtp_fanout_host_rw below.
 *
 * srtp_fanout_device: every array is a device pointer, the call asynchronous on
 * `stream` like srtp_transform_device, under the engine's lock while it
 * enqueues.  src_len and src_status are read on the device, so the len and
 * status arrays of a preceding srtp_transform_device(reverse = 1) on the same
 * stream feed them without a synchronise: a received bundle is forwarded with
 * no host round trip.  The caller guarantees for both segments what
 * srtp_transform_device asks of its regions, and that the two segments do not
 * overlap; an out-of-range src_idx is not the caller's guarantee (skipped,
 * above).  m = 0 with n > 0 is SRTP_EINVAL.
 *
 * srtp_fanout_host: host pointers.  Checks both region tables as
 * srtp_transform_host does, src_idx[j] in [0, m) and m >= 1 (else SRTP_EINVAL,
 * nothing launched), copies only the source segment and the small arrays to
 * the device, expands and protects there, copies the destination segment, len
 * and status back and synchronises.  The host destination segment is OUTPUT
 * ONLY: after the call the bytes [off[j], off[j] + len[j]) of the entries with
 * SRTP_STATUS_OK are defined, every other byte of it is unspecified (whatever
 * it held before is lost).
 *
 * n = 0 is SRTP_OK with nothing launched; a NULL engine SRTP_EINVAL before any
 * device call. */
int srtp_fanout_device(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                       const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                       uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                       const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                       int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                     const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                     uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                     size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                     const uint32_t *flags, int32_t *status, uint32_t n);
/* Cumulative since engine creation: fan-out calls that were enqueued, their
 * sources (m) and destination entries (n), the entries skipped for their index
 * or their source's status (not those the caller flagged), and the source bytes
 * srtp_fanout_host copied host-to-device. */
typedef struct {
    uint64_t calls, sources, destinations, skipped, src_bytes_h2d;
} srtp_fanout_stats;
int srtp_engine_fanout_stats(srtp_engine *e, srtp_fanout_stats *out);
/* The rule of one destination entry (host only; fanout_job.h, the text k_fanout
 * compiles): the bytes to copy (a multiple of 16, never past either region
 * rounded up to 16), the entry's length and flags word, and by_source = 1 when
 * it is skipped for its index or its source's status.  src_len, src_cap and
 * src_status matter only for an index in [0, m). */
typedef struct {
    int32_t copy_bytes, len_out;
    uint32_t flags_out;
    int32_t by_source;
} srtp_fanout_plan;
int srtp_fanout_job(int32_t src_idx, int32_t m, int32_t src_len, int32_t src_cap, int32_t src_status,
                    int32_t dst_cap, uint32_t flags, srtp_fanout_plan *out);

/* Fan-out with per-destination rewriting.  In the reference each stream's send
 * chain holds ptTransformEngine and ssrcRewritingEngine in front of the SRTP
 * transformer (MediaStreamImpl.java:986-1035): a simulcast or last-N bridge
 * sends every peer the packet under that peer's target SSRC, with a continuous
 * sequence number, sometimes a replaced timestamp, and the peer's payload type
 * (ExtendedSequenceNumberInterval.rewriteRTP, through four RawPacket setters).
 * The state machine that chooses the values stays on the host; it hands the
 * device one record per destination entry, values in host byte order, and the
 * expansion writes them into entry j's copy before the protect chain parses it
 * -- the SRTP context is found under the rewritten SSRC and the ROC follows the
 * rewritten sequence number, as for a host-made copy the setters were applied
 * to.  The rewrite applies to entry j exactly when the entry is not skipped,
 * rewrite[j].mask & 0xF is non-zero and at least 12 bytes are copied
 * (min(src_len, src_cap, cap[j]) >= 12); otherwise the copy is what
 * srtp_fanout_device makes.  The source segment is never written.  Mask bits
 * above 0xF: srtp_fanout_host_rw refuses them (SRTP_EINVAL, nothing launched);
 * on the device route, where the records are not read back, they are ignored.
 * `reserved` is ignored.  The rule knows nothing of the transformer's kind: for
 * an SRTCP transformer only mask 0 makes sense, which is the caller's
 * responsibility.  The RTX OSN and the FEC SN base are srtp_fanout_device_pay's
 * (below); RTCP rewriting is not done here: such a packet goes to its peer as
 * a host-made copy. */
typedef struct { uint32_t mask, ssrc, timestamp; uint16_t seq; uint8_t pt, reserved; } srtp_fanout_rewrite;
#define SRTP_REWRITE_SSRC 0x1u       /* RawPacket.setSSRC:           bytes 8..11 = ssrc, big-endian */
#define SRTP_REWRITE_SEQ 0x2u        /* RawPacket.setSequenceNumber: bytes 2..3  = seq, big-endian */
#define SRTP_REWRITE_TIMESTAMP 0x4u  /* RawPacket.setTimestamp:      bytes 4..7  = timestamp, big-endian */
#define SRTP_REWRITE_PT 0x8u         /* RawPacket.setPayloadType:    byte 1 = (byte 1 & 0x80) | (pt & 0x7F) */
/* srtp_fanout_device / srtp_fanout_host with one more argument after flags:
 * rewrite, n records (k_fanout_rw).  rewrite == NULL is the call without it,
 * exactly.  Device route: a device array, 16-byte aligned (else SRTP_EINVAL
 * before any launch).  Host route: a host array, staged like src_idx. */
int srtp_fanout_device_rw(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                          const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                          uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                          const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                          const srtp_fanout_rewrite *rewrite, int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host_rw(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                        const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                        uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                        size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                        const uint32_t *flags, const srtp_fanout_rewrite *rewrite, int32_t *status, uint32_t n);
/* The rewrite rule of one destination entry (host only; fanout_job.h, the text
 * k_fanout_rw compiles): the first seven arguments are srtp_fanout_job's;
 * words_in are the three little-endian 32-bit words of the copy's header bytes
 * 0..11.  applies = 1 and words = the patched words when the rewrite applies,
 * else applies = 0 and words = words_in. */
typedef struct {
    int32_t applies;
    uint32_t words[3];
} srtp_fanout_rewrite_plan;
int srtp_fanout_rewrite_job(int32_t src_idx, int32_t m, int32_t src_len, int32_t src_cap, int32_t src_status,
                            int32_t dst_cap, uint32_t flags, const srtp_fanout_rewrite *rewrite,
                            const uint32_t *words_in, srtp_fanout_rewrite_plan *out);

/* Fan-out that stamps abs-send-time per destination.  The third engine the
 * reference puts in front of a stream's SRTP transformer is absSendTimeEngine
 * (MediaStreamImpl.java:1018-1035): AbsSendTimeEngine.replaceAbsSendTime
 * (AbsSendTimeEngine.java:86-152) walks the packet's one-byte header-extension
 * elements, and the first element whose ID is the stream's negotiated
 * abs-send-time ID, if its len field is 2, gets its three data bytes
 * overwritten with the local send time in 6.18 fixed point.  Those bytes are
 * authenticated (and AAD under AES-GCM), so they are written into entry j's
 * copy before the protect chain sees it.  The host hands the device one record
 * per destination entry: the 24-bit value (the top 8 bits are ignored), the
 * peer's ID and `on`.  The record is on when on != 0; an id above 15 never
 * matches (as in the reference, whose ID is an int compared with a nibble) and
 * behaves as off; `reserved` is ignored.
 *
 * With c = min(src_len, src_cap, cap[j]) and b the copy's bytes, the stamp
 * applies only if the entry is not skipped, the record is on, c >= 12,
 * (b[0] >> 6) == 2 and b[0] & 0x10.  The walk is the reference's, with a buffer
 * that ends where the c copied bytes end and Java's signed bytes:
 *   p = 12 + 4 * (b[0] & 15) + 2
 *   if p + 1 < c:  lw = (sbyte(b[p]) << 8) | sbyte(b[p + 1]);  nbytes = 4 * (1 + lw)
 *     p += 2; inner = 0
 *     while p < c and inner < nbytes:
 *       if (b[p] >> 4) == id:  stamp b[p + 1 .. p + 3] if (b[p] & 15) == 2 and p + 3 < c;  stop
 *       inner += (b[p] & 15) + 2;  p += (b[p] & 15) + 2
 * with what follows from it: a length field with a byte >= 0x80 walks nothing;
 * the "defined by profile" word is not looked at; the walk may step four bytes
 * past the extension and stamp there; a padding byte advances by 2; the first
 * element with the ID ends the walk whatever its len.  Every stamped byte is
 * one the copy wrote; the source segment is never written.  Nothing is
 * inserted: a packet without the element leaves as it came.  The rewrite
 * records touch bytes 1..11 and the walk reads b[0] of them only, so the two
 * apply in either order. */
typedef struct { uint32_t value; uint8_t id, on; uint16_t reserved; } srtp_fanout_abs_send_time;
/* srtp_fanout_device_rw / srtp_fanout_host_rw with one more argument after
 * rewrite: stamp, n records (k_fanout_ast).  stamp == NULL is the _rw call,
 * exactly.  With stamp set, rewrite may be NULL (stamp only) or set (both).
 * Device route: a device array, 8-byte aligned (else SRTP_EINVAL before any
 * launch).  Host route: a host array, staged like src_idx and rewrite. */
int srtp_fanout_device_ast(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                           const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                           uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                           const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                           const srtp_fanout_rewrite *rewrite, const srtp_fanout_abs_send_time *stamp,
                           int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host_ast(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                         const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                         uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                         size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                         const uint32_t *flags, const srtp_fanout_rewrite *rewrite,
                         const srtp_fanout_abs_send_time *stamp, int32_t *status, uint32_t n);
/* The stamp rule of one destination entry (host only; fanout_job.h, the text
 * k_fanout_ast compiles) over the caller's bytes: pkt[0 .. bound) is the
 * packet (reads past bound, which cannot happen for bound >= min(src_len,
 * src_cap, dst_cap), answer 0); the next seven arguments are srtp_fanout_job's.
 * *out = the offset of the first of the three stamped bytes, or -1. */
int srtp_fanout_ast_job(const uint8_t *pkt, uint32_t bound, int32_t src_idx, int32_t m, int32_t src_len,
                        int32_t src_cap, int32_t src_status, int32_t dst_cap, uint32_t flags,
                        const srtp_fanout_abs_send_time *stamp, int32_t *out);

/* Fan-out that patches the payload per destination: the last per-peer bytes of
 * ExtendedSequenceNumberInterval.rewriteRTP (ExtendedSequenceNumberInterval.java:
 * 163-229), which the rewriting engine writes before SRTP sees the packet.
 *   RTX  rewriteRTX (:261-284): pkt.setOriginalSequenceNumber((short) sn) is
 *        writeShort(getHeaderLength(), sn) (RawPacket.java:1018-1022,
 *        1334-1337): two bytes, big-endian, at the start of the payload -- the
 *        peer's rewritten number of the original packet.
 *   FEC  rewriteFEC (:346-386), plain or as the matching block of a RED packet
 *        (rewriteRED, :307-333): the SN base of the FEC header, buf[off + 2]
 *        and buf[off + 3].
 * The payload is ciphered (under AES-GCM sealed), so the bytes are written into
 * entry j's copy before the protect chain runs.  The host keeps everything
 * that chooses values -- the rewriter's intervals, rtx2primary / ssrc2fec /
 * ssrc2red, the RED block walk, getHeaderLength() of the source -- and hands
 * the device one 8-byte record per destination entry with two patches: b0[0],
 * b0[1] go to packet bytes at0, at0 + 1, then b1[0], b1[1] to at1, at1 + 1.
 * An all-zero record does nothing.
 *
 * With c = min(src_len, src_cap, cap[j]): a patch is on exactly when the entry
 * is not skipped, at >= 12 and c > at.  A patch below byte 12 is refused whole
 * (those bytes are the setters').  Of a patch that is on, byte i of {at, at + 1}
 * is written iff i < c, as the reference's two writeByte calls: at == c - 1
 * writes the first byte only.  No byte is written that the copy did not write;
 * the source segment is never written.  Order within an entry: patch 0, patch 1
 * (where they overlap patch 1 wins), then the abs-send-time stamp (where they
 * overlap the stamp wins; its walk reads the patched bytes) -- the reference's
 * chain, ssrcRewritingEngine (MediaStreamImpl.java:998) in front of
 * absSendTimeEngine (:1018-1020).  The rewrite records touch bytes 1..11 only
 * and apply in either order.  The record carries bytes and has no opinion on
 * what they mean. */
typedef struct srtp_fanout_payload {
    uint16_t at0; uint8_t b0[2];   /* patch 0: b0[0], b0[1] go to packet bytes at0, at0 + 1; at0 == 0: off */
    uint16_t at1; uint8_t b1[2];   /* patch 1, likewise, applied after patch 0 */
} srtp_fanout_payload;
/* srtp_fanout_device_ast / srtp_fanout_host_ast with one more argument after
 * stamp: pay, n records (k_fanout_pay).  pay == NULL is the _ast call, exactly.
 * With pay set, rewrite and stamp may each be NULL.  Device route: a device
 * array, 8-byte aligned (else SRTP_EINVAL before any launch).  Host route: a
 * host array, staged like src_idx, rewrite and stamp.  Replaces, per copy,
 * rewriteRTX's setOriginalSequenceNumber (ExtendedSequenceNumberInterval.java:
 * 261-284) and rewriteFEC's two stores (:346-386). */
int srtp_fanout_device_pay(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                           const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                           uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                           const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                           const srtp_fanout_rewrite *rewrite, const srtp_fanout_abs_send_time *stamp,
                           const srtp_fanout_payload *pay, int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host_pay(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                         const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                         uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                         size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                         const uint32_t *flags, const srtp_fanout_rewrite *rewrite,
                         const srtp_fanout_abs_send_time *stamp, const srtp_fanout_payload *pay,
                         int32_t *status, uint32_t n);
/* The patch rule of one destination entry (host only; fanout_job.h, the text
 * k_fanout_pay compiles) over the caller's piece: the first seven arguments are
 * srtp_fanout_job's; words_in are the four little-endian 32-bit words of bytes
 * 16 q .. 16 q + 15 of the copy (q >= 0).  words_out = the piece with patch 0,
 * then patch 1 applied: what RawPacket.writeShort (RawPacket.java:1334-1337)
 * and rewriteFEC's stores (ExtendedSequenceNumberInterval.java:383-384) leave of
 * it, under the rules above. */
int srtp_fanout_pay_job(int32_t src_idx, int32_t m, int32_t src_len, int32_t src_cap, int32_t src_status,
                        int32_t dst_cap, uint32_t flags, const srtp_fanout_payload *pay, int32_t q,
                        const uint32_t *words_in, uint32_t *words_out);

/* Fan-out that strips or adds RED (RFC 2198) per destination: the one engine of
 * the peer's send chain that moves the payload.  Chrome sends video as
 * single-block RED; for a peer that did not negotiate it the reference runs
 * REDFilterTransformEngine.transform (transform/REDFilterTransformEngine.java:
 * 95-145), which takes the one-byte RED header out, and for a peer that did,
 * when the source sent none, REDTransformEngine.transform (transform/
 * REDTransformEngine.java:151-182, in the chain at MediaStreamImpl.java:993-996),
 * which puts it in.  One 4-byte record per destination entry says which:
 *   SRTP_RED_OFF    nothing (the reference's payload type -1, "disabled")
 *   SRTP_RED_STRIP  a version-2 packet whose PT is red_pt, that is no RTCP by
 *                   the predicate's test (byte 1 in 200..211, marker included)
 *                   and whose header ends inside the packet loses the byte at
 *                   getHeaderLength(); its 7 low bits become the PT.  Length - 1.
 *   SRTP_RED_WRAP   a version-2 packet gets the byte (PT & 0x7F) at
 *                   getHeaderLength() and red_pt as its PT.  Length + 1; where
 *                   that exceeds cap[j] nothing is moved and the entry ends
 *                   SRTP_STATUS_DROP_INVALID like a host-made copy.
 * Where the reference throws -- a header that ends past the packet's bytes, an
 * extension length word past them, a RED header with F set (at this revision a
 * multi-block packet always throws, red_job.h says why) -- the packet is lost
 * there and the entry is dropped here: nothing is copied, len[j] = 0, the entry
 * ends SRTP_STATUS_SKIPPED and touches no context.  The step is asked for only
 * when the entry is not skipped and the whole packet is there (min(src_len,
 * src_cap, cap[j]) == src_len >= 12); otherwise the entry is the _pay call's.
 * RED runs first: rewrite[j], pay[j] (its offsets in the new packet's
 * coordinates) and stamp[j] apply to the packet RED left, with its new length,
 * as ssrcRewritingEngine stands behind RED (MediaStreamImpl.java:998).  The
 * source segment is never written.  red_job.h states the rule line by line. */
#define SRTP_RED_OFF 0
#define SRTP_RED_STRIP 1
#define SRTP_RED_WRAP 2
typedef struct { uint8_t mode, red_pt, reserved[2]; } srtp_fanout_red;
/* red_out[j]: what became of entry j */
#define SRTP_RED_UNTOUCHED 0
#define SRTP_RED_STRIPPED 1
#define SRTP_RED_WRAPPED 2
#define SRTP_RED_DROPPED (-1)
/* srtp_fanout_device_pay / srtp_fanout_host_pay with two more arguments after
 * pay: red, n records (k_fanout_red), and red_out, n result codes (may be
 * NULL).  red == NULL is the _pay call, exactly (red_out is then not written).
 * With red set, rewrite, stamp and pay may each be NULL.  Device route: red is a
 * device array, 4-byte aligned (else SRTP_EINVAL before any launch), red_out n
 * bytes on the device; a record with mode > 2, red_pt > 127 or non-zero
 * reserved bytes switches its entry's step off (result 0).  Host route: host
 * arrays, the records staged like pay and red_out copied back with len and
 * status; such a record is refused (SRTP_EINVAL, nothing launched). */
int srtp_fanout_device_red(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                           const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                           uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                           const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                           const srtp_fanout_rewrite *rewrite, const srtp_fanout_abs_send_time *stamp,
                           const srtp_fanout_payload *pay, const srtp_fanout_red *red, int8_t *red_out,
                           int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host_red(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                         const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                         uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                         size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                         const uint32_t *flags, const srtp_fanout_rewrite *rewrite,
                         const srtp_fanout_abs_send_time *stamp, const srtp_fanout_payload *pay,
                         const srtp_fanout_red *red, int8_t *red_out, int32_t *status, uint32_t n);
/* Counters of the _red calls with red set, cumulative since engine creation:
 * the calls and the entries stripped, wrapped and dropped. */
typedef struct {
    uint64_t calls, stripped, wrapped, dropped;
} srtp_fanout_red_stats;
int srtp_engine_fanout_red_stats(srtp_engine *e, srtp_fanout_red_stats *out);
/* The RED rule of one destination entry (host only; red_job.h, the text
 * k_fanout_red compiles) over the caller's bytes: pkt[0 .. min(src_len, src_cap,
 * dst_cap)) is the source packet as far as it is copied; the next seven
 * arguments are srtp_fanout_job's.  result: SRTP_RED_UNTOUCHED / _STRIPPED /
 * _WRAPPED / _DROPPED; h: getHeaderLength() where stripped or wrapped, else 0;
 * len_out: the entry's length behind the step; shift: -1, +1 or 0. */
typedef struct {
    int32_t result, h, len_out, shift;
} srtp_fanout_red_plan;
int srtp_fanout_red_job(const uint8_t *pkt, int32_t src_idx, int32_t m, int32_t src_len, int32_t src_cap,
                        int32_t src_status, int32_t dst_cap, uint32_t flags, const srtp_fanout_red *red,
                        srtp_fanout_red_plan *out);

/* Fan-out that makes ulpfec packets (RFC 5109, one level, short mask) per
 * destination: the last engine in front of SRTP whose work grows with the
 * payload, FECTransformEngine with its FECSender (transform/fec/FECSender.java,
 * in the chain at MediaStreamImpl.java:988-991).  A destination entry can be an
 * FEC entry: it has no source (src_idx[j] == -1), is made from up to 16 member
 * entries of the same call and is then protected like any other entry.  Its
 * plaintext is, byte for byte, what FECSender.FECPacket yields when addMedia is
 * called on the members in list order and then finish() (:319-412), the
 * members taken as they stand in the destination segment behind all their
 * records (RED, rewrite, pay, stamp) and in front of the protect chain:
 *   bytes 0-11   0x80, pt & 0x7F, the last member's sequence number + 1, the
 *                last member's timestamp, ssrc
 *   bytes 12-19  the XOR of the members' bytes 0-7, bytes 14-15 then the first
 *                member's sequence number (SN base)
 *   bytes 20-25  the XOR of len - 12, max(len - 12) (the protection length),
 *                ((1 << count) - 1) << (16 - count)
 *   bytes 26..   the XOR of the members' bytes from 12 on, a shorter member
 *                contributing zeros; the length is 26 + the protection length
 * mode SRTP_FEC_RED applies REDTransformEngine.transform to that packet (byte 12
 * = pt, byte 1 = red_pt, everything from byte 12 on one byte up, length + 1).
 * The reference runs the FEC engine in front of RED and SSRC rewriting and
 * repairs only the SN base afterwards; here the XOR is over the packets the
 * peer gets, as if the engine stood directly in front of SRTP.  For a peer
 * without records the two coincide.  fec_job.h states the rule line by line.
 *
 * members[first .. first + count) are indices of destination entries.  An entry
 * whose record is on is refused -- len[j] = 0, SKIP in the engine's flags word,
 * SRTP_STATUS_SKIPPED, no context touched -- when count is outside 1..16, first
 * + count > n_members, pt > 127, red_pt > 127 with mode 2, mode > 2, its own
 * src_idx is not -1 (what the expansion copied there stays in its region), or a
 * member is outside [0, n), has a record that is on, carries SKIP after the
 * expansion, has not 12 <= len <= cap, or is not version 2.  A made entry's own
 * rewrite, stamp, pay and red records are ignored; len[j] is 26 (27) + the
 * protection length even past cap[j]: then only the bytes below cap[j] rounded
 * up to 16 are stored and the entry ends SRTP_STATUS_DROP_INVALID like a
 * host-made copy.  Two FEC entries may share members. */
#define SRTP_FEC_OFF 0
#define SRTP_FEC_PLAIN 1
#define SRTP_FEC_RED 2
typedef struct { uint32_t first, ssrc; uint8_t count, pt, red_pt, mode; } srtp_fanout_fec;
/* fec_out[j]: 0 the record is off or the caller flagged the entry SKIP */
#define SRTP_FEC_NONE 0
#define SRTP_FEC_MADE 1
#define SRTP_FEC_REFUSED (-1)
/* srtp_fanout_device_red / srtp_fanout_host_red with four more arguments after
 * red_out: fec, n records; members and n_members; fec_out, n result codes (may
 * be NULL).  fec == NULL is the _red call, exactly.  Device route: fec and
 * members are device arrays, 4-byte aligned (else SRTP_EINVAL before any
 * launch); nothing is read back.  Host route: src_idx[j] == -1 is accepted
 * exactly for entries whose record is on; a record or member that the rule
 * would refuse for its fields or indices is SRTP_EINVAL with nothing launched;
 * fec_out is copied back with len and status. */
int srtp_fanout_device_fec(srtp_engine *e, const uint8_t *src_seg, const uint32_t *src_off,
                           const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                           uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                           const uint32_t *off, uint32_t *len, const uint32_t *cap, const uint32_t *flags,
                           const srtp_fanout_rewrite *rewrite, const srtp_fanout_abs_send_time *stamp,
                           const srtp_fanout_payload *pay, const srtp_fanout_red *red, int8_t *red_out,
                           const srtp_fanout_fec *fec, const int32_t *members, uint32_t n_members,
                           int8_t *fec_out, int32_t *status, uint32_t n, void *stream);
int srtp_fanout_host_fec(srtp_engine *e, const uint8_t *src_seg, size_t src_seg_bytes, const uint32_t *src_off,
                         const uint32_t *src_len, const uint32_t *src_cap, const int32_t *src_status,
                         uint32_t m, const int32_t *src_idx, const int32_t *tids, int32_t tid, uint8_t *seg,
                         size_t seg_bytes, const uint32_t *off, uint32_t *len, const uint32_t *cap,
                         const uint32_t *flags, const srtp_fanout_rewrite *rewrite,
                         const srtp_fanout_abs_send_time *stamp, const srtp_fanout_payload *pay,
                         const srtp_fanout_red *red, int8_t *red_out, const srtp_fanout_fec *fec,
                         const int32_t *members, uint32_t n_members, int8_t *fec_out, int32_t *status,
                         uint32_t n);
/* Counters of the _fec calls with fec set, cumulative since engine creation:
 * the calls, the entries made and refused, and the member bytes XORed (len - 4
 * per member of a made entry: eight header bytes and the payload).
 * srtp_fanout_stats.skipped does not count entries whose record is on. */
typedef struct {
    uint64_t calls, made, refused, member_bytes;
} srtp_fanout_fec_stats;
int srtp_engine_fanout_fec_stats(srtp_engine *e, srtp_fanout_fec_stats *out);
/* The FEC rule of one entry (host only; fec_job.h, the text k_fanout_fec
 * compiles) over the caller's member bytes: member i is bytes[at[i] .. at[i] +
 * lens[i]), i < rec->count, with no flag, no record and cap = lens[i]; the
 * entry's own src_idx is -1 and n_members is rec->first + rec->count.  *code
 * gets SRTP_FEC_MADE or SRTP_FEC_REFUSED (SRTP_FEC_NONE for mode 0), *len_out
 * the packet's length, and out[0 .. min(*len_out, out_cap)) its bytes, built
 * piece by piece as the kernel builds them. */
int srtp_fanout_fec_job(const srtp_fanout_fec *rec, const uint8_t *bytes, const uint32_t *at, const uint32_t *lens,
                        uint8_t *out, uint32_t out_cap, int32_t *len_out, int8_t *code);

/* Recovery of lost media packets from ulpfec (RFC 5109, one level, short or
 * long mask) on the device: the receive half of the FEC engine, FECReceiver's
 * Reconstructor (transform/fec/FECReceiver.java, setFecPacket :472-520 and
 * recover :527-596), over the tables of a bundle that has been unprotected.
 * The operation is stateless: record r names one FEC entry (`fec`) and up to 64
 * candidate entries cand[first .. first + count) of the same tables -- the
 * entries that may be its media packets, which the host can name from the clear
 * RTP headers before the unprotect has run -- and the receiver's SSRC.  An
 * entry, the FEC packet or a candidate, counts iff its index lies in [0, n),
 * status[i] is SRTP_STATUS_OK (status == NULL: every entry) and 12 <= len[i] <=
 * cap[i] <= 65535; a candidate that does not count is absent (a packet that
 * failed authentication was not received).  Of candidates with equal sequence
 * numbers the one latest in the list stands.  fec_rx_job.h states the rule line
 * by line, with the reference's quirk kept (a key base + k above 65535 is never
 * found) and the defined deviations (a read at or past the FEC packet's len
 * refuses the record).  code[r]:
 *   SRTP_FECRX_OFF        on == 0: nothing else of the record is read
 *   SRTP_FECRX_RECOVERED  exactly one protected packet was missing; it is made
 *   SRTP_FECRX_COMPLETE   none was missing: the FEC packet is of no further use
 *   SRTP_FECRX_WAIT       more than one is missing
 *   SRTP_FECRX_PARTIAL    protectionLength < lengthRecovery: the reference
 *                         logs and returns null
 *   SRTP_FECRX_REFUSED    count > 64, first + count > n_cand, the FEC entry
 *                         does not count, or its header or payload does not lie
 *                         below its len
 * Recovered: out_len[r] = the packet's length, out_status[r] = SRTP_STATUS_OK
 * and the bytes stand at out_seg + out_off[r]; a packet longer than out_cap[r]
 * keeps its length, ends SRTP_STATUS_DROP_INVALID and only the pieces below
 * out_cap[r] rounded up to 16 are stored.  Any other code: out_len[r] = 0,
 * out_status[r] = SRTP_STATUS_SKIPPED and no byte of out_seg is written.  The
 * arrays out_seg, out_off, out_len, out_cap and out_status are what
 * srtp_fanout_device* takes as sources.  The input segment is never written;
 * bytes of an output region at or past out_len[r] are unspecified.
 *
 * Device route: every array is device memory, rec and cand 4-byte aligned
 * (else SRTP_EINVAL before any launch); asynchronous on `stream`; status and
 * len are read on the device, so the arrays of a srtp_transform_device(reverse
 * = 1) enqueued before on the same stream feed it with no synchronise.  Nothing
 * is read back, no engine scratch is touched and no other stream's bundle is
 * waited for.  Host route: both region tables are validated, a record or
 * candidate index the rule would refuse is SRTP_EINVAL with nothing launched,
 * and out_len, out_status, code and the output segment are copied back. */
typedef struct { int32_t fec; uint32_t first, ssrc; uint8_t count, on; uint16_t reserved; } srtp_fec_recover;
#define SRTP_FECRX_OFF 0
#define SRTP_FECRX_RECOVERED 1
#define SRTP_FECRX_COMPLETE 2
#define SRTP_FECRX_WAIT 3
#define SRTP_FECRX_PARTIAL 4
#define SRTP_FECRX_REFUSED (-1)
int srtp_fec_recover_device(srtp_engine *e, const uint8_t *seg, const uint32_t *off, const uint32_t *len,
                            const uint32_t *cap, const int32_t *status, uint32_t n, const srtp_fec_recover *rec,
                            uint32_t n_rec, const int32_t *cand, uint32_t n_cand, uint8_t *out_seg,
                            const uint32_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *out_status,
                            int8_t *code, void *stream);
int srtp_fec_recover_host(srtp_engine *e, const uint8_t *seg, size_t seg_bytes, const uint32_t *off,
                          const uint32_t *len, const uint32_t *cap, const int32_t *status, uint32_t n,
                          const srtp_fec_recover *rec, uint32_t n_rec, const int32_t *cand, uint32_t n_cand,
                          uint8_t *out_seg, size_t out_seg_bytes, const uint32_t *out_off, const uint32_t *out_cap,
                          uint32_t *out_len, int32_t *out_status, int8_t *code);
/* Counters of the recover calls, cumulative since engine creation: the calls,
 * and, counted by the kernel, the records that were on, how they ended, and the
 * member bytes XORed (len - 4 per needed member of a recovered record).  The
 * kernel's counts are those of the calls that have completed: synchronise the
 * streams of the device route first. */
typedef struct {
    uint64_t calls, records, recovered, complete, waiting, partial, refused, member_bytes;
} srtp_fec_recover_stats;
int srtp_engine_fec_recover_stats(srtp_engine *e, srtp_fec_recover_stats *out);
/* The recovery rule of one record (host only; fec_rx_job.h, the text
 * k_fec_recover compiles): the FEC packet is fec[0 .. fec_len), candidate i is
 * bytes[at[i] .. at[i] + lens[i]), i < rec->count, each with status OK and cap =
 * its length; rec->fec and rec->first are not read.  *code gets the
 * SRTP_FECRX_* code, *len_out the packet's length (0 unless recovered) and
 * out[0 .. min(*len_out, out_cap)) its bytes, built piece by piece as the
 * kernel builds them. */
int srtp_fec_recover_job(const srtp_fec_recover *rec, const uint8_t *fec, uint32_t fec_len, const uint8_t *bytes,
                         const uint32_t *at, const uint32_t *lens, uint8_t *out, uint32_t out_cap, int32_t *len_out,
                         int8_t *code);

/* The engine's own non-blocking stream, created with the engine so that each
 * engine gets a hardware queue of its own (streams created later may share
 * one, which serialises them): srtp_transform_host and the pipeline run their
 * kernels on it, and srtp_transform_device callers can. */
void *srtp_engine_stream(srtp_engine *e);
/* stream == NULL: wait for every bundle this engine has enqueued (any stream) */
int srtp_engine_sync(srtp_engine *e, void *stream);
/* returns 1 and fills *out if the transformer has a context for ssrc, else 0 */
int srtp_get_context_state(srtp_engine *e, int32_t transformer, uint32_t ssrc,
                           srtp_ctx_state *out);
/* number of live contexts in the engine's table */
int64_t srtp_engine_num_contexts(srtp_engine *e);

/* Per-engine counters (SURVEY.md 5 metrics).  The reference keeps none for
 * auth / replay failures (SRTPCryptoContext.java:635-638 logs at debug level)
 * and counts only exceptions (SinglePacketTransformer.java:42,54-59,140-148);
 * here every final per-packet status is counted, cumulatively since engine
 * creation.  ctx_overflow counts packets that found no free context slot (they
 * get SRTP_STATUS_DROP_NO_CONTEXT); ctx_live / ctx_tombstones / ctx_slots
 * describe the context table at the time of the call. */
typedef struct {
    uint64_t bundles, packets;           /* bundles / packets submitted */
    uint64_t status[SRTP_NUM_STATUS];    /* final statuses, indexed by SRTP_STATUS_* */
    uint64_t roc_rechecks;               /* unprotect tags re-checked under a ROC the walk
                                            guessed differently from the speculation */
    uint64_t repaired;                   /* packets whose speculative decryption was redone */
    uint64_t ctx_overflow;               /* packets refused a new context: table full */
    uint64_t ctx_live, ctx_tombstones, ctx_slots;
    uint64_t rehashes;                   /* context-table rebuilds (tombstone cleanup) */
    uint64_t chain_stalls;               /* walk tiles that gave up waiting for a long chain's
                                            state from the tiles before (never expected; the
                                            chain is then walked serially from the exact state
                                            by the last tile to finish, so results stay exact) */
    uint64_t long_walked;                /* packets of chains of 32+ packets that the wave-wide
                                            speculation could not take and were walked one at
                                            a time (the slow path) */
    uint64_t holes;                      /* bundle-former holes: SRTP_PKT_FLAG_SKIP entries of no
                                            transformer (tid < 0) that srtp_aggregator_* seals
                                            unclaimed; not in status[SRTP_STATUS_SKIPPED] */
    uint64_t small_bundles;              /* bundles run by k_small: every phase in one launch */
    uint64_t small_aead_bundles;         /* ... by its GCM instance (an engine that holds an
                                            AES-GCM key set); not in small_bundles */
} srtp_stats;
int srtp_engine_stats(srtp_engine *e, srtp_stats *out);

/* Test hooks (0 in production): SRTP_DEBUG_FORCE_CHAIN_STALL makes every third
 * chain-pass walk tile give up its look-back at once, which exercises the
 * stall fix-up (srtp_stats.chain_stalls) that a tile preempted for seconds
 * would take.  Results must not change. */
#define SRTP_DEBUG_FORCE_CHAIN_STALL 0x1u
/* SRTP_DEBUG_FORCE_WIDE runs bundles of every size on the split path (the
 * cipher and the MAC as two kernels, which bundles of 2048-65536 packets take
 * when every key set is AES-CM or NULL cipher with HMAC-SHA1), so that every
 * parity case exercises it; SRTP_DEBUG_NO_WIDE keeps every bundle off it
 * (A/B measurements).  Results must not change. */
#define SRTP_DEBUG_FORCE_WIDE 0x2u
#define SRTP_DEBUG_NO_WIDE 0x4u
/* SRTP_DEBUG_NO_SMALL keeps bundles of up to 255 packets off k_small (the
 * whole bundle -- parse, sort, walk, keystream, MAC -- in one workgroup and
 * one launch, which such bundles take under the split path's key-set rule);
 * FORCE_WIDE and NO_WIDE keep them off it too. */
#define SRTP_DEBUG_NO_SMALL 0x8u
/* The AES-GCM passes of a bundle of up to srtp_gcm_wave_max() packets run a wave
 * per packet (k_gcm_wave: GHASH as a sum over the powers of H, a block per
 * lane), larger ones a lane per packet (k_gcm).  SRTP_DEBUG_NO_GCM_WAVE always
 * takes the lane kernel, SRTP_DEBUG_FORCE_GCM_WAVE always the wave kernel (so
 * that every parity case reaches it; A/B measurements).  Results must not
 * change. */
#define SRTP_DEBUG_NO_GCM_WAVE 0x10u
#define SRTP_DEBUG_FORCE_GCM_WAVE 0x20u
int32_t srtp_gcm_wave_max(void);
/* An engine that holds an AES-GCM key set runs a bundle of up to
 * srtp_small_aead_max() packets in one launch (k_small's GCM instance,
 * srtp_stats.small_aead_bundles), larger ones on the multi-kernel path: the
 * instance checks the GCM tags before the walk in one workgroup, a wave per
 * packet, and loses to the chain once a wave has more than one.
 * SRTP_DEBUG_FORCE_SMALL lifts the limit to k_small's own 255 packets (so that
 * every parity case reaches the instance's several workgroups; A/B
 * measurements); NO_SMALL, the WIDE hooks and the GCM_WAVE hooks keep every
 * bundle off it.  Results must not change. */
#define SRTP_DEBUG_FORCE_SMALL 0x40u
int32_t srtp_small_aead_max(void);
/* Unprotect of AES-GCM packets on the multi-kernel path opens a packet in one
 * pass over its bytes: the pass before the walk checks the tag under the ROC
 * guess and deciphers in the same trip (k_gcm<open>), the pass after the walk
 * only repairs the packets whose verdict the walk overturned (k_gcm<fix>: a
 * replay, a packet behind a throwing one under abort-on-error -- deciphered
 * text put back as the ciphertext that came in).  Results are those of the
 * two-pass route (tag check, walk, decipher) to the bit.  It is the default
 * where it measured faster, clean and with 2.5 % replays and forgeries: on the
 * wave route for bundles of srtp_gcm_open_wave_min() to srtp_gcm_open_wave_max()
 * packets (4096 to 8192); on the lane route for bundles of
 * srtp_gcm_open_lane_min() packets and more, which is INT32_MAX -- it won there
 * only on clean bundles of 2^18, so the lane route stays on two passes.
 * SRTP_DEBUG_NO_GCM_SPEC keeps every bundle on the two-pass route (A/B
 * measurements, parity, fallback); SRTP_DEBUG_FORCE_GCM_SPEC puts every bundle
 * of the multi-kernel path on the one-pass route, whichever kernels it takes
 * (the parity tests; the only way to the lane kernels' one-pass modes).
 * Neither flag changes which bundles k_small takes. */
#define SRTP_DEBUG_NO_GCM_SPEC 0x80u
#define SRTP_DEBUG_FORCE_GCM_SPEC 0x100u
int32_t srtp_gcm_open_lane_min(void);
int32_t srtp_gcm_open_wave_min(void);
int32_t srtp_gcm_open_wave_max(void);
/* opened: packets deciphered together with their tag check; restored: opened
 * packets put back as ciphertext after the walk (not in srtp_stats.repaired);
 * late: packets deciphered after the walk although the bundle took the
 * one-pass route (a ROC the walk re-checked, a header whose extension length
 * is negative).  Cumulative; all 0 on an engine without AES-GCM key sets and
 * under SRTP_DEBUG_NO_GCM_SPEC. */
typedef struct {
    uint64_t opened, restored, late;
} srtp_gcm_stats;
int srtp_engine_gcm_stats(srtp_engine *e, srtp_gcm_stats *out);
int srtp_engine_set_debug(srtp_engine *e, uint32_t flags);
/* The AES-GCM switch (RFC 7714 profiles, see SRTP_AESGCM_ENCRYPTION): off on a
 * new engine.  While on, srtp_factory_create accepts the GCM policy shape for
 * its SRTP and / or SRTCP policy; turning it off again refuses new such
 * factories and leaves existing ones working.  An engine that holds a GCM
 * factory still runs its bundles of up to srtp_small_aead_max() packets -- the
 * per-packet callers' lone calls among them, direct mode included -- in one
 * launch (k_small's GCM instance, srtp_stats.small_aead_bundles), as long as
 * its other key sets are AES-CM / NULL cipher + HMAC-SHA1 ones; its larger
 * bundles run on the multi-kernel path (no split path). */
int srtp_engine_enable_aead(srtp_engine *e, int32_t on);
/* The room, in bytes, that the per-packet paths leave behind a packet for
 * protect's trailer: 16 (SRTCP's E|index word and a 12-byte tag), or 20 when
 * `aead` is non-zero (GCM SRTCP: a 16-byte tag and the word).
 * srtp_engine_trailer_room: that of the engine's AES-GCM switch as it stands
 * (16 for NULL).  An aggregator (and so every queue on it) and a RawPacket
 * batch sample it once, when they are created: turn the switch on before
 * creating them.  One created earlier keeps 16, and protecting a GCM SRTCP
 * packet through it answers SRTP_STATUS_ERR_CAPACITY; an engine without the
 * switch packs exactly the bundles it always did. */
int32_t srtp_trailer_room(int32_t aead);
int32_t srtp_engine_trailer_room(srtp_engine *e);

/* Context-state export / import: lets a stream's ROC, s_l,
 * replay window and SRTCP indices follow it to another engine or GPU (SSRC
 * re-sharding, failover) or survive a transformer rebuild.  The reference keeps
 * this state inside SRTPCryptoContext (srtp/SRTPCryptoContext.java:96-135) with
 * no API for it; DtlsPacketTransformer rebuilds contexts from scratch on rekey
 * (tf/dtls/DtlsPacketTransformer.java:614-642).
 *
 * srtp_export_contexts writes up to `max` (ssrc, state) pairs of the
 * transformer's contexts and sets *count to the number it has (which may
 * exceed max).  srtp_set_context_state creates or overwrites the transformer's
 * context for ssrc with *st (key_set ignored); its session keys are those of
 * the transformer's forward (forward = 1) or reverse factory, which must be
 * open.  Both synchronise the engine's device. */
int srtp_export_contexts(srtp_engine *e, int32_t transformer, uint32_t *ssrcs,
                         srtp_ctx_state *states, uint32_t max, uint32_t *count);
int srtp_set_context_state(srtp_engine *e, int32_t transformer, uint32_t ssrc, int32_t forward,
                           const srtp_ctx_state *st);

/* Exact context snapshots (the dispatcher's abort rollback, dispatch.cpp):
 * srtp_contexts_save copies the contexts (tids[i], ssrcs[i]) -- their whole
 * record, key set included, as an opaque srtp_ctx_raw -- and sets present[i]
 * to 0 where the transformer has no context for ssrcs[i].  srtp_contexts_restore
 * puts such a snapshot back: the context is created or overwritten where
 * present[i] != 0 and removed where present[i] == 0, so the table is as it
 * was when the snapshot was taken.  The (tid, ssrc) pairs of one restore call
 * must be distinct.  Both wait for the engine's enqueued bundles.  No
 * reference API (SRTPCryptoContext's state is private). */
typedef struct {
    uint64_t w[4];
} srtp_ctx_raw;
int srtp_contexts_save(srtp_engine *e, uint32_t n, const int32_t *tids, const uint32_t *ssrcs,
                       srtp_ctx_raw *out, int32_t *present);
int srtp_contexts_restore(srtp_engine *e, uint32_t n, const int32_t *tids, const uint32_t *ssrcs,
                          const srtp_ctx_raw *in, const int32_t *present);

/* Per-stage kernel timing with HIP events recorded on the bundle's stream
 * (measurement hook for bench.py; off by default). */
#define SRTP_STAGE_PARSE 0
#define SRTP_STAGE_SORT 1
#define SRTP_STAGE_VERIFY 2
#define SRTP_STAGE_WALK 3
#define SRTP_STAGE_PROTECT 4
#define SRTP_STAGE_DECRYPT 5
#define SRTP_NUM_STAGES 6
int srtp_engine_set_timing(srtp_engine *e, int32_t enable);
/* Waits for the recorded events, adds each stage's total milliseconds and
 * bundle count since the last read into ms[] / count[], and resets. */
int srtp_engine_read_timing(srtp_engine *e, double *ms, uint64_t *count);

/* Host bundle pipeline (SURVEY.md 8d end-to-end timing, 8f.2 bundle former):
 * `depth` slots of pinned host memory the caller packs bundles into directly
 * (the RawPacket[] -> packed-segment marshalling a JNI shim does; see
 * INTEGRATION.md), each moved H2D on a copy stream, processed by the engine on
 * its stream in submission order, and moved D2H on a second copy stream, so
 * slot i's copies overlap slot j's kernels.  Replaces the reference's
 * per-packet calls through PacketTransformer.transform/reverseTransform
 * (transform/PacketTransformer.java:28-53) fed 1-element arrays by
 * RTPConnectorInputStream.java:425-452 / RTPConnectorOutputStream.java:268-300.
 *
 * srtp_pipeline_slot_get returns slot i's pinned arrays (seg holds seg_cap
 * bytes; the per-packet arrays hold max_packets entries).  srtp_pipeline_submit
 * enqueues slot i's first n packets (seg_bytes of segment) as one bundle for
 * transformer `tid`, or per packet from slot.tids when use_tids != 0; flags
 * are passed when use_flags != 0.  It first waits for the slot's previous
 * bundle.  srtp_pipeline_wait blocks until slot i's results (seg, len, status)
 * are back in its pinned arrays.  Packet regions are validated as in
 * srtp_transform_host. */
typedef struct srtp_pipeline srtp_pipeline;
typedef struct {
    uint8_t *seg;
    size_t seg_cap;
    uint32_t *off, *len, *cap, *flags;
    int32_t *tids, *status;
    uint32_t max_packets;
} srtp_pipeline_slot;
int srtp_pipeline_create(srtp_engine *e, uint32_t max_packets, size_t max_seg_bytes,
                         int32_t depth, srtp_pipeline **out);
void srtp_pipeline_destroy(srtp_pipeline *pl);
int srtp_pipeline_slot_get(srtp_pipeline *pl, int32_t slot, srtp_pipeline_slot *out);
int srtp_pipeline_submit(srtp_pipeline *pl, int32_t slot, int32_t reverse, int32_t use_tids,
                         int32_t tid, int32_t use_flags, uint32_t n, size_t seg_bytes);
int srtp_pipeline_wait(srtp_pipeline *pl, int32_t slot);
/* 1 when slot's bundle has come back (srtp_pipeline_wait then returns without
 * blocking) or none is in flight, 0 while it is still running, < 0 on error. */
int srtp_pipeline_query(srtp_pipeline *pl, int32_t slot);
/* srtp_pipeline_create with flags.  SRTP_PIPE_ONE_STREAM puts the copies on
 * the engine's own stream instead of two copy streams of the pipeline's: a
 * bundle's H2D, kernels and D2H then run in order with no cross-stream
 * events.  For engines that share a GPU (several dispatcher shards or
 * aggregator lanes on one device): every stream maps onto one of the device's
 * few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and a queue that
 * holds one engine's kernel waiting on its copy event stalls every other
 * engine's work behind it.  Without the flag, bundles of up to 1 MB still
 * copy on the engine's stream (their round trip is fixed costs, and two
 * cross-stream events are among them); larger ones use the copy streams. */
#define SRTP_PIPE_ONE_STREAM 0x1u
/* SRTP_PIPE_POLL_CROWDED: a wait on this pipeline polls the bundle's event
 * (sleeping between polls) instead of spinning in hipEventSynchronize while
 * more than 4 threads of the process
 * wait on such pipelines -- for one pipeline per caller thread (the 1-packet
 * RawPacket path): 64 spinning callers took the host's cores from the threads
 * enqueueing the next bundles.  Few waiters keep the spin's quicker wake-up. */
#define SRTP_PIPE_POLL_CROWDED 0x2u
int srtp_pipeline_create_ex(srtp_engine *e, uint32_t max_packets, size_t max_seg_bytes, int32_t depth,
                            uint32_t flags, srtp_pipeline **out);
/* srtp_pipeline_submit with the bundle's abort-on-throw chosen per bundle:
 * abort_on_error = -1 the engine's option, 1 SinglePacketTransformer's abort of
 * a throwing transformer's later packets (one RawPacket[] call), 0 none (every
 * packet its own 1-element array: the bundle former's bundles).  One engine
 * can so serve both kinds of call with the same contexts. */
int srtp_pipeline_submit_ex(srtp_pipeline *pl, int32_t slot, int32_t reverse, int32_t use_tids,
                            int32_t tid, int32_t use_flags, uint32_t n, size_t seg_bytes,
                            int32_t abort_on_error);

/* Registered host memory: the zero-copy host path.  srtp_host_register pins
 * [ptr, ptr + bytes) for DMA by every device of the process (hipHostRegister,
 * portable) -- a long-lived buffer pool, e.g. the JVM's direct ByteBuffers a
 * media server receives into, registered once.  Ranges may not overlap;
 * srtp_host_unregister takes the pointer that was registered, and the caller
 * must not unregister or free a range while a call uses it.
 * srtp_host_is_registered tells whether [ptr, ptr + bytes) lies inside one
 * registered range.  srtp_host_alloc allocates such a range as pinned memory
 * of the engine's own (hipHostMalloc; freed with srtp_host_free): the DMA
 * engines read it at the full PCIe rate, while registered pageable memory of
 * 4-KB pages may move slower.  A JVM would wrap it as a direct ByteBuffer
 * (NewDirectByteBuffer).  No reference API: the reference's packets are heap
 * byte[]s copied by every JNI call (src/native/openssl/).
 *
 * srtp_pipeline_submit_host is srtp_pipeline_submit_ex with the segment read
 * from, and written back to, registered caller memory (host_seg, seg_bytes)
 * instead of the slot's seg: the slot's per-packet arrays still describe the
 * bundle (off relative to host_seg).  srtp_dispatch_transform_host does this
 * by itself for every chunk of a shard whose packets lie back to back in a
 * registered segment, so a one-shard dispatcher moves a registered bundle
 * with no host copy at all.
 *
 * srtp_pipeline_submit_gather is the form for packets scattered over
 * registered memory (a shard's share of an interleaved bundle): the slot's
 * arrays lay the bundle out in the slot (off, cap, ...), and packet j's region
 * (cap[j] rounded to 16 bytes) is read by the GPU from host_base + src_off[j]
 * over PCIe before the bundle runs, and written back there after it --
 * [host_base, host_base + host_bytes) must be registered; at most 32768
 * packets.  srtp_dispatch_transform_host / _submit_host use it for every
 * chunk of a registered bundle whose packets do not lie back to back, so a
 * many-shard dispatcher moves a registered bundle with no host copy of its
 * bytes either.  (Round 6; the registration maps the memory for the GPU.) */
int srtp_host_register(void *ptr, size_t bytes);
int srtp_host_unregister(void *ptr);
int srtp_host_alloc(size_t bytes, void **out);
int srtp_host_free(void *ptr);
int32_t srtp_host_is_registered(const void *ptr, size_t bytes);
int srtp_pipeline_submit_host(srtp_pipeline *pl, int32_t slot, int32_t reverse, int32_t use_tids,
                              int32_t tid, int32_t use_flags, uint32_t n, size_t seg_bytes,
                              int32_t abort_on_error, uint8_t *host_seg);
int srtp_pipeline_submit_gather(srtp_pipeline *pl, int32_t slot, int32_t reverse, int32_t use_tids,
                                int32_t tid, int32_t use_flags, uint32_t n, size_t seg_bytes,
                                int32_t abort_on_error, uint8_t *host_base, size_t host_bytes,
                                const uint32_t *src_off);

/* Bundle aggregator over the pipeline: per-packet submits
 * from any number of threads become bundles.  Replaces the reference's
 * one-packet-at-a-time calls through the transform chain
 * (RTPConnectorInputStream.java:425-452 receive, RTPConnectorOutputStream.java
 * :268-300,652-830 send; each a 1-element array through
 * SinglePacketTransformer.java:121-216).
 *
 * srtp_aggregator_submit copies one packet (len bytes; protect leaves the
 * aggregator's trailer room behind it, srtp_aggregator_trailer_room: 16 bytes,
 * or 20 on an engine with AES-GCM on) into the open bundle of its direction; a bundle is
 * sealed when it holds max_packets packets or max_bytes bytes, when its oldest
 * packet has waited deadline_us, or on srtp_aggregator_flush.  Sealed bundles
 * run in sealing order; when one completes, `cb` is called (on the
 * aggregator's dispatch thread) once per packet, in bundle order, with the
 * packet's cookie, final status (SRTP_STATUS_*; -1 if the bundle could not be
 * submitted) and processed bytes, valid only during the call.  So packets
 * of one direction -- and thus of one transformer -- complete in the order
 * they were accepted (per submitting thread when several threads submit).
 * Every packet is its own 1-element array, as in the reference: one packet's
 * exception (SRTP_STATUS_ERR_MALFORMED) does not stop the others (the bundles
 * run without abort-on-throw whatever the engine's abort_on_error, so one
 * engine or dispatcher serves this and srtp_rawpacket_transform alike).  When
 * every slot is sealed or in flight, submit blocks (backpressure).  flush
 * seals the open bundles and waits until every packet accepted before it has
 * completed; destroy refuses new submits (SRTP_EINVAL, also from callbacks),
 * waits until every accepted packet has completed, then stops the threads.  Submits take no lock: each thread fills its own block of 16
 * entries of the open bundle (one compare-and-swap per block on the bundle,
 * one per packet on the thread's own block), so producers do not share a
 * written cache line per packet; entries of a block left unclaimed when the
 * bundle is sealed go to the engine as SRTP_PKT_FLAG_SKIP holes (counted as
 * SKIPPED in srtp_engine_stats, no callback).  Callbacks may submit (e.g.
 * forward a received packet); a submit made from a callback never blocks: when
 * no slot is free the packet is parked and placed in the first slot the
 * aggregator frees, ahead of other producers.  Producers outside callbacks
 * leave one slot of each lane (depth - 1 usable) for callback submits.  flush
 * from a callback returns SRTP_EINVAL and destroy from a callback does
 * nothing.  cb may be NULL for an aggregator that serves only synchronous
 * calls (srtp_aggregator_transform); srtp_aggregator_submit then returns
 * SRTP_EINVAL. */
typedef struct srtp_aggregator srtp_aggregator;
#define SRTP_AGG_SEAL_IDLE 0x1 /* seal a lane's open bundle at once while the lane has no
                                  bundle in flight (adaptive: bundles grow with the load) */
typedef struct {
    uint32_t max_packets; /* per bundle, default 1<<14 */
    size_t max_bytes;     /* per bundle (segment), default 24 MB */
    uint32_t deadline_us; /* default 1000 */
    int32_t depth;        /* pipeline slots (3..16), default 4 */
    uint32_t flags;       /* SRTP_AGG_*, default SRTP_AGG_SEAL_IDLE */
} srtp_aggregator_opts;
typedef void (*srtp_aggregator_cb)(void *user, uint64_t cookie, int32_t status, const uint8_t *data,
                                   uint32_t len);
int srtp_aggregator_opts_default(srtp_aggregator_opts *opts);
int srtp_aggregator_create(srtp_engine *e, const srtp_aggregator_opts *opts, srtp_aggregator_cb cb,
                           void *user, srtp_aggregator **out);
int srtp_aggregator_submit(srtp_aggregator *a, int32_t reverse, int32_t tid, const uint8_t *pkt,
                           uint32_t len, uint32_t flags, uint64_t cookie);
int srtp_aggregator_flush(srtp_aggregator *a);
int srtp_aggregator_stats(srtp_aggregator *a, uint64_t *accepted, uint64_t *completed,
                          uint64_t *bundles);
void srtp_aggregator_destroy(srtp_aggregator *a);
/* The synchronous per-packet call: SinglePacketTransformer.transform /
 * reverseTransform(RawPacket) (SinglePacketTransformer.java:113,169 as
 * SRTPTransformer.java:185-219 / SRTCPTransformer.java:175-207 implement
 * it) from any number of threads at once.  The packet -- copy_len bytes of
 * pkt (what lies behind its length, e.g. an extension header the reference
 * reads past it), RTP/RTCP length len, buffer room cap >= len (in-place
 * protect needs 16 bytes behind the packet) -- joins the lane's open bundle
 * like a submit, so concurrent callers share bundles; the call returns when
 * its bundle has completed, with the packet's final status, length and bytes
 * (max(len, *out_len) bytes to out, which holds at least cap bytes).  It
 * never calls the aggregator's callback.  With SRTP_AGG_SEAL_IDLE a call into
 * an idle lane is sealed at once, so a lone caller waits one GPU round trip
 * and concurrent callers coalesce behind the bundle in flight; deadline_us
 * bounds the wait for a seal otherwise.  Not from a callback (SRTP_EINVAL). */
int srtp_aggregator_transform(srtp_aggregator *a, int32_t reverse, int32_t tid, const uint8_t *pkt,
                              uint32_t copy_len, uint32_t len, uint32_t cap, uint32_t flags,
                              uint8_t *out, int32_t *status, uint32_t *out_len);
/* Transformer t's kind (read without a lock after the first call) and, when
 * fwd_rtcp_tag_len != NULL, its forward factory's SRTCP tag length
 * (srtp_transformer_info on the first shard). */
int srtp_aggregator_transformer_info(srtp_aggregator *a, int32_t t, int32_t *kind,
                                     int32_t *fwd_rtcp_tag_len);
/* The trailer room the aggregator sampled when it was created
 * (srtp_engine_trailer_room of its engine, or of its dispatcher's shards): what
 * srtp_aggregator_submit adds to a protect packet's length for its region, and
 * what srtp_rawpacket_transform_one / srtp_rawpacket_submit use on it. */
int32_t srtp_aggregator_trailer_room(srtp_aggregator *a);

/* Completion queues: the asynchronous per-packet call.  The
 * reference's connectors already queue: RTPConnectorOutputStream.write hands
 * packets to a send thread that drains them (RTPConnectorOutputStream.java
 * :652-830, runInSendThread :775), and the receive thread hands on every
 * datagram (RTPConnectorInputStream.java:425-452,780-806).  Such a thread owns
 * a queue, submits every packet it has and reaps the results, so it keeps
 * many packets in flight instead of one.
 *
 * srtp_queue_submit: one packet as srtp_aggregator_transform takes it
 * (copy_len bytes of pkt, length len, room cap >= copy_len) joins its lane's
 * open bundle (the aggregator's sealing rules apply); cookie is the caller's.
 * A packet with SRTP_PKT_FLAG_SKIP, or with len > cap (RawPacket.isInvalid),
 * completes at once with SRTP_STATUS_SKIPPED / SRTP_STATUS_DROP_INVALID and
 * no bytes.  Returns SRTP_EAGAIN when max_inflight packets are outstanding;
 * when no slot is free it waits for one, but only until the queue's oldest
 * outstanding packet has completed (then SRTP_EAGAIN: the caller reaps and
 * submits again), or at once when the last reap's completions are still
 * held (not released).
 *
 * srtp_queue_reap: up to max completions, in SUBMISSION order (so per
 * transformer and SSRC the reference's order), into out; with wait != 0 it
 * blocks until at least one is there when any packet is outstanding.
 * Returns the count.  out[i].data points at the packet's processed bytes in
 * the aggregator's pinned slot (max(len, in_len) bytes, within cap; NULL for
 * packets completed at submit) and stays valid until the next reap or
 * destroy of this queue (or srtp_queue_release): reaping releases the
 * previous reap's packets, and a slot is reused only when every packet of it
 * has been released -- so a caller done with its completions releases them
 * (srtp_queue_release) rather than holding slots until its next reap.
 *
 * A queue belongs to one thread at a time (submit and reap are not
 * thread-safe on one queue); queues of one aggregator are independent.
 * Packets of one direction and lane still run in the order the aggregator
 * accepted them across all its producers.  srtp_queue_destroy waits for the
 * queue's outstanding packets; every queue must be destroyed before its
 * aggregator (srtp_aggregator_destroy waits for that).  Not from an
 * aggregator callback (SRTP_EINVAL). */
typedef struct srtp_queue srtp_queue;
typedef struct {
    uint64_t cookie;     /* as submitted */
    int32_t status;      /* SRTP_STATUS_* (-1: the bundle could not be submitted) */
    uint32_t len;        /* the packet's length after the call */
    uint32_t in_len;     /* its length at submit */
    int32_t reverse;     /* as submitted */
    int32_t tid;         /* as submitted */
    const uint8_t *data; /* processed bytes (see above) */
} srtp_completion;
int srtp_queue_create(srtp_aggregator *a, uint32_t max_inflight, srtp_queue **out);
int srtp_queue_submit(srtp_queue *q, int32_t reverse, int32_t tid, const uint8_t *pkt, uint32_t copy_len,
                      uint32_t len, uint32_t cap, uint32_t flags, uint64_t cookie);
int srtp_queue_reap(srtp_queue *q, srtp_completion *out, uint32_t max, int32_t wait);
/* Releases the last reap's completions (their data pointers become invalid). */
void srtp_queue_release(srtp_queue *q);
/* packets submitted and not yet reaped */
int32_t srtp_queue_outstanding(srtp_queue *q);
srtp_aggregator *srtp_queue_aggregator(srtp_queue *q);
void srtp_queue_destroy(srtp_queue *q);

/* In-process multi-GPU dispatcher (SURVEY.md 8b engine_create(devices, opts),
 * 8e): one engine per shard, shard i on device devices[i] (a device may host
 * several shards).  A host bundle is split by shard = srtp_shard_of(SSRC)
 * (RTP: RawPacket.getSSRC, RTCP: getRTCPSSRC) -- SRTP contexts are per
 * (transformer, SSRC), SRTPTransformer.java:62,152-175, so each GPU owns its
 * SSRCs' state and nothing crosses GPUs.  Every shard's sub-bundle keeps
 * bundle order; statuses, lengths and packet bytes are scattered back in
 * place.  Results are identical to one engine processing the whole bundle,
 * including SinglePacketTransformer's abort-on-throw
 * (SinglePacketTransformer.java:134-155,190-210), which the dispatcher
 * reproduces across shards by rolling back a throwing transformer's later
 * packets and the contexts they touched (see dispatch.cpp): a bundle costs at
 * most two runs per shard however many of its packets throw.  Factories and
 * transformers are created on every shard with the same ids as one engine
 * would assign.  srtp_dispatch_plan is the host-only split (no GPU needed):
 * per packet its shard (-1: handled without an engine) and whether it could
 * throw (may_throw, only with abort_on_error); it returns 2 if some packet
 * could throw (the bundle needs context snapshots), else 1.  kinds[t] =
 * transformer t's kind, tag_mask bit T = some policy has tag length T. */
typedef struct srtp_dispatch srtp_dispatch;
int32_t srtp_shard_of(uint32_t ssrc, int32_t n_shards);
int32_t srtp_dispatch_plan(int32_t n_shards, int32_t abort_on_error, int32_t reverse,
                           const int32_t *kinds, int32_t n_transformers, uint32_t tag_mask,
                           const int32_t *tids, int32_t tid, const uint8_t *seg, size_t seg_bytes,
                           const uint32_t *off, const uint32_t *len, const uint32_t *cap,
                           const uint32_t *flags, uint32_t n, int32_t *shard, int32_t *may_throw);
int srtp_dispatch_create(const int32_t *devices, int32_t n_shards, const srtp_engine_opts *opts,
                         srtp_dispatch **out);
void srtp_dispatch_destroy(srtp_dispatch *d);
const char *srtp_dispatch_last_error(srtp_dispatch *d);
int32_t srtp_dispatch_num_shards(srtp_dispatch *d);
srtp_engine *srtp_dispatch_engine(srtp_dispatch *d, int32_t shard);
/* srtp_engine_enable_aead on every shard's engine */
int srtp_dispatch_enable_aead(srtp_dispatch *d, int32_t on);
int srtp_dispatch_factory_create(srtp_dispatch *d, int32_t sender, const uint8_t *master_key,
                                 int32_t key_len, const uint8_t *master_salt, int32_t salt_len,
                                 const srtp_policy *srtp, const srtp_policy *srtcp, int32_t *out);
int srtp_dispatch_factory_close(srtp_dispatch *d, int32_t factory);
int srtp_dispatch_transformer_create(srtp_dispatch *d, int32_t kind, int32_t fwd, int32_t rev,
                                     int32_t *out);
int srtp_dispatch_transformer_set_factory(srtp_dispatch *d, int32_t transformer, int32_t factory,
                                          int32_t forward);
int srtp_dispatch_transformer_close(srtp_dispatch *d, int32_t transformer);
int srtp_dispatch_transform_host(srtp_dispatch *d, int32_t reverse, const int32_t *tids, int32_t tid,
                                 uint8_t *seg, size_t seg_bytes, const uint32_t *off, uint32_t *len,
                                 const uint32_t *cap, const uint32_t *flags, int32_t *status,
                                 uint32_t n);
/* Asynchronous host bundles (no reference API: RTPConnectorOutputStream's
 * send thread, RTPConnectorOutputStream.java:268-300, hands each packet on
 * and goes back to its queue).  srtp_dispatch_submit_host does the work of
 * srtp_dispatch_transform_host but returns once the bundle's last chunks are
 * on their way to the GPUs, with a ticket; srtp_dispatch_wait_host(ticket)
 * returns when its statuses, lengths and bytes are in the caller's arrays,
 * with the bundle's result.  The arrays must stay valid, and untouched by the
 * caller, until that wait returns.  The next submit overlaps its packing and
 * H2D with the previous bundle's last D2H.  Bundles run in submission order
 * on every shard (each context sees its packets in that order, as from
 * synchronous calls), and a synchronous call is ordered with them too.  Every
 * ticket must be waited for (at most 64 may be outstanding: SRTP_EAGAIN
 * beyond); waiting for one also completes -- but does not consume -- the
 * bundles submitted before it.  A bundle with a packet that could throw under
 * abort-on-throw (the rollback above) runs to completion inside its submit.
 * srtp_dispatch_destroy completes bundles never waited for. */
int srtp_dispatch_submit_host(srtp_dispatch *d, int32_t reverse, const int32_t *tids, int32_t tid,
                              uint8_t *seg, size_t seg_bytes, const uint32_t *off, uint32_t *len,
                              const uint32_t *cap, const uint32_t *flags, int32_t *status, uint32_t n,
                              uint64_t *ticket);
int srtp_dispatch_wait_host(srtp_dispatch *d, uint64_t ticket);
int srtp_dispatch_get_context_state(srtp_dispatch *d, int32_t transformer, uint32_t ssrc,
                                    srtp_ctx_state *out);
int srtp_dispatch_set_context_state(srtp_dispatch *d, int32_t transformer, uint32_t ssrc,
                                    int32_t forward, const srtp_ctx_state *st);
/* srtp_stats summed over the shards */
int srtp_dispatch_stats(srtp_dispatch *d, srtp_stats *out);
/* srtp_gcm_stats summed over the shards */
int srtp_dispatch_gcm_stats(srtp_dispatch *d, srtp_gcm_stats *out);
/* Host time of srtp_dispatch_transform_host since creation, in ns: [0] plan
 * and split, [1] packing into the shards' pinned slots and enqueueing each
 * chunk's copies and kernels, [2] waiting for the
 * shards' bundles (H2D + kernels + D2H), [3] scattering results back (1-3
 * summed over the shards' worker threads), [4] wall time of the calls, [5]
 * number of calls. */
int srtp_dispatch_host_times(srtp_dispatch *d, uint64_t ns[6]);
/* The shard a packet of transformer `tid` goes to (as srtp_dispatch_transform_host
 * routes it: its SSRC's shard, shard 0 for a packet shorter than 12 bytes);
 * -1 for an unknown transformer.  Does not wait for bundles in flight. */
int32_t srtp_dispatch_route(srtp_dispatch *d, int32_t tid, const uint8_t *pkt, uint32_t len);
/* 1 when the reference could throw on this packet of a transformer of `kind`
 * (SRTP_KIND_*) -- the per-packet test of srtp_dispatch_plan, a superset of the
 * engine's SRTP_STATUS_ERR_MALFORMED: RawPacket.getHeaderLength,
 * SRTPCipherCTR.process / SRTPCipherF8.process bounds, RawPacket.getSRTCPIndex
 * -- for policies whose tag lengths are in tag_mask (bit T: tag length T, bit
 * 0: NULL authentication); pkt holds cap bytes (a smaller cap only widens the
 * superset: the header may then seem to end past it).  0 for a
 * packet that is skipped or invalid (len < 12 or len > cap).  Host only. */
int32_t srtp_packet_may_throw(int32_t kind, int32_t reverse, const uint8_t *pkt, uint32_t len, uint32_t cap,
                              uint32_t flags, uint32_t tag_mask);
/* The aggregator over a dispatcher: one lane per shard (its own pinned slots
 * and dispatch thread); each packet goes to the lane of its shard, so
 * per-packet submits from one process reach every GPU.  Callbacks of
 * different shards run concurrently on the lanes' threads; the packets of
 * one shard -- hence of one (transformer, SSRC) context -- and one direction
 * complete in the order they were accepted.  opts apply per lane; every
 * shard's engine must have abort_on_error = 0. */
int srtp_aggregator_create_dispatch(srtp_dispatch *d, const srtp_aggregator_opts *opts,
                                    srtp_aggregator_cb cb, void *user, srtp_aggregator **out);

/* RawPacket[] marshalling for the Java drop-in (the JNI shim
 * src/native/srtp_mi355x/ calls exactly this).  PacketTransformer.transform /
 * reverseTransform(RawPacket[]) as SinglePacketTransformer.java:121-216 runs
 * it: element i is bufs[i] (NULL: a null element, skipped) with the RawPacket's
 * buffer length, offset, length and flags (SRTP_PKT_FLAG_SKIP: the packet
 * predicate rejected it; FLAG_DISCARD / FLAG_SILENCE as RawPacket.getFlags).
 * Packs the elements into a bundle of transformer tids[i] (tids == NULL: tid),
 * runs it, and writes each result back into its buffer in place, as the
 * reference leaves it: status[i] (drops: the caller replaces the element with
 * null; the RawPacket keeps what was done to it -- e.g. the shrink of a failed
 * tag check), length[i] updated.  need_len[i] != 0 where the reference
 * allocates a new buffer -- RawPacket.append without room after the payload
 * (RawPacket.java:203-220), and RawPacket.grow for every SRTCP protect
 * (:885-893): the caller allocates need_len[i] bytes, copies the result from
 * srtp_rawpacket_result to offset 0, and sets buffer / offset 0 / length.
 * *thrown = the first element the reference throws on (SRTP_STATUS_ERR_MALFORMED;
 * -1: none): every element was written back, the thrower keeps its partial
 * mutation, its transformer's later packets are NOT_PROCESSED and untouched,
 * and the caller rethrows.  A batch is the staging of one calling thread
 * (pinned memory for an engine); results stay valid until its next call. */
typedef struct srtp_rawpacket_batch srtp_rawpacket_batch;
int srtp_rawpacket_batch_create(srtp_engine *e, srtp_rawpacket_batch **out);
int srtp_rawpacket_batch_create_dispatch(srtp_dispatch *d, srtp_rawpacket_batch **out);
void srtp_rawpacket_batch_destroy(srtp_rawpacket_batch *b);
int srtp_rawpacket_transform(srtp_rawpacket_batch *b, int32_t reverse, const int32_t *tids, int32_t tid,
                             uint8_t *const *bufs, const uint32_t *buf_len, const uint32_t *offset,
                             uint32_t *length, const uint32_t *flags, int32_t *status,
                             uint32_t *need_len, uint32_t n, int32_t *thrown);
int srtp_rawpacket_result(srtp_rawpacket_batch *b, uint32_t i, const uint8_t **data, uint32_t *len);
/* Arrays of up to 8192 packets none of which can throw (srtp_packet_may_throw)
 * then go through a completion queue on aggregator a -- whose lanes must be
 * over the batch's engine or dispatcher -- instead of a bundle of their own:
 * concurrent callers' arrays share bundles, and no caller waits behind
 * another's GPU round trip.  The results are the same (no packet can throw, so
 * abort-on-throw has nothing to stop); other arrays keep the batch's own
 * bundle.  The queue lives for one srtp_rawpacket_transform call, so a batch
 * holds nothing on the aggregator between calls (srtp_aggregator_destroy
 * waits only for calls in progress).  If the call fails part-way, the elements
 * that did not complete get SRTP_STATUS_ERR_INTERNAL and are left untouched.
 * a = NULL turns this off. */
int srtp_rawpacket_batch_set_aggregator(srtp_rawpacket_batch *b, srtp_aggregator *a);
/* One RawPacket through SinglePacketTransformer.transform / reverseTransform
 * (RawPacket) (SinglePacketTransformer.java:113,169; every
 * RTPConnector*Stream call and DtlsPacketTransformer.transformSrtp,
 * DtlsPacketTransformer.java:1544-1564, hands the transformer one packet at
 * a time), coalesced with concurrent callers' packets through the aggregator
 * (srtp_aggregator_transform).  The element marshalling and write-back are
 * srtp_rawpacket_transform's for an array of one: buf (NULL: a null element)
 * of buf_len bytes holds the packet at offset with *length bytes; *status,
 * *length and the bytes in buf are updated in place; *need_len != 0 where the
 * reference reallocates (RawPacket.append / grow), the result then being the
 * first *need_len bytes of grow, which must hold grow_cap >= *length + the
 * aggregator's trailer room (16 or 20) bytes and at least the bytes from offset to the end of buf (min 65535).
 * SRTP_STATUS_ERR_MALFORMED: the reference throws (the packet keeps its
 * partial mutation); the caller rethrows. */
int srtp_rawpacket_transform_one(srtp_aggregator *a, int32_t reverse, int32_t tid, uint8_t *buf,
                                 uint32_t buf_len, uint32_t offset, uint32_t *length, uint32_t flags,
                                 int32_t *status, uint32_t *need_len, uint8_t *grow, uint32_t grow_cap);
/* The per-packet call, asynchronous (a connector's send thread
 * or receive loop keeping many packets in flight): one RawPacket element as
 * srtp_rawpacket_transform_one takes it (buf NULL or flags with
 * SRTP_PKT_FLAG_SKIP: SKIPPED; *length past the buffer: DROP_INVALID, both
 * completed at once) submitted to queue q (srtp_queue_submit; SRTP_EAGAIN:
 * reap first).  Each completion reaped from q then goes back into its
 * RawPacket by srtp_rawpacket_complete, given the buffer's bytes after the
 * packet's offset (avail): *need_len == 0: *copy_len bytes of c->data go back
 * in place at the offset; else the reference allocates a new buffer of
 * *need_len bytes (RawPacket.append / grow) at offset 0 that receives
 * *copy_len bytes of c->data.  Either way the RawPacket's length becomes
 * c->len; SRTP_STATUS_ERR_MALFORMED is the reference's throw (the packet keeps
 * its partial mutation), other non-OK statuses its null. */
int srtp_rawpacket_submit(srtp_queue *q, int32_t reverse, int32_t tid, const uint8_t *buf, uint32_t buf_len,
                          uint32_t offset, uint32_t length, uint32_t flags, uint64_t cookie);
int srtp_rawpacket_complete(srtp_queue *q, const srtp_completion *c, uint32_t avail, uint32_t *copy_len,
                            uint32_t *need_len);
/* Devices the engine can use (hipGetDeviceCount; 0 without a GPU): what the
 * Java drop-in sizes its dispatcher with. */
int32_t srtp_device_count(void);

/* Control-plane crypto without a GPU (used by CPU-side tests): RFC 3711 4.3
 * session keys exactly as SRTPCryptoContext.deriveSrtpKeys (rtcp = 0) /
 * SRTCPCryptoContext.deriveSrtcpKeys (rtcp = 1). */
int srtp_derive_session_keys(const uint8_t master_key[16], const uint8_t master_salt[14],
                             int32_t rtcp, uint8_t enc_key[16], uint8_t auth_key[20],
                             uint8_t salt_key[14]);
/* The same for a 16- or 32-byte master key (AES-128 / AES-256 PRF, RFC 6188
 * 4.1): enc_key receives key_len bytes. */
int srtp_derive_session_keys_n(const uint8_t *master_key, int32_t key_len,
                               const uint8_t master_salt[14], int32_t rtcp, uint8_t *enc_key,
                               uint8_t auth_key[20], uint8_t salt_key[14]);
/* The same with the policy's cipher as the PRF: AES for SRTP_AESCM / AESF8 /
 * NULL, Twofish for SRTP_TWOFISH(F8)_ENCRYPTION (BaseSRTPCryptoContext.java
 * :197-226 keys that cipher with the master key). */
int srtp_derive_session_keys_for(int32_t enc_type, const uint8_t *master_key, int32_t key_len,
                                 const uint8_t master_salt[14], int32_t rtcp, uint8_t *enc_key,
                                 uint8_t auth_key[20], uint8_t salt_key[14]);
/* The same with an auth key of auth_len bytes (1..64; 32 for ZRTP's Skein
 * policies, whose authKeyLength is 32: ZRTPTransformEngine.java:867-872). */
int srtp_derive_session_keys_auth(int32_t enc_type, const uint8_t *master_key, int32_t key_len,
                                  const uint8_t master_salt[14], int32_t rtcp, uint8_t *enc_key,
                                  uint8_t *auth_key, int32_t auth_len, uint8_t salt_key[14]);
/* Skein-512 (version 1.3) keyed with key[0..key_len) (key_len 0: the plain
 * hash), out_bits (1..512) output bits: the tag bccontrib's SkeinMac computes
 * for SRTPPolicy.SKEIN_AUTHENTICATION (BaseSRTPCryptoContext.java:244-248). */
int srtp_skein512_mac(const uint8_t *key, int32_t key_len, int32_t out_bits, const uint8_t *msg,
                      size_t n, uint8_t *out);
/* One block of the policy's cipher: AES-128/256 (key_len 16 / 32) or Twofish
 * (enc_type SRTP_TWOFISH*, key_len 16 / 24 / 32). */
int srtp_block_encrypt(int32_t enc_type, const uint8_t *key, int32_t key_len, const uint8_t in[16],
                       uint8_t out[16]);

/* AES-GCM one-shot on the host (NIST SP 800-38D with a 96-bit IV and a
 * 16-byte tag, the form RFC 7714 5 uses): seals data[0, len) in place under
 * key (16 or 32 bytes) with the additional data aad and writes tag; with
 * `open` set it opens instead -- returns 1 on a tag mismatch, leaving data
 * untouched, else deciphers.  GHASH runs by Shoup's 4-bit method: the
 * 16-entry table a GPU pass would take per key set (host_crypto.h). */
int srtp_aes_gcm(int32_t open, const uint8_t *key, int32_t key_len, const uint8_t iv[12],
                 const uint8_t *aad, int32_t aad_len, uint8_t *data, int32_t len, uint8_t tag[16]);

/* The device twin of srtp_aes_gcm: n packets on the engine's device, one key
 * (16 or 32 bytes) for the batch.  Packet i is seg[off[i] .. off[i] +
 * aad_len[i] + len[i]), AAD first; iv holds n x 12 bytes, tag n x 16.
 * open = 0: seal in place, write tag (result may be NULL).  open = 1:
 * result[i] = 1 and the data left untouched on a mismatch, else 0 and
 * deciphered.  No byte of seg outside the packets is read or written; packets
 * must not overlap; any alignment (4-byte aligned data runs faster).  All
 * arrays are device pointers; key is a host pointer, expanded on the host and
 * passed in the kernel's arguments.  Enqueued on `stream` (NULL: the device's
 * default stream); the results are ready once the stream reaches that point.
 * Stateless: touches no factory, transformer or context of the engine, which
 * names the device.  Like every call on an engine it holds the engine's lock
 * while it enqueues (not while the kernel runs), so it is serialised against
 * bundle submits from other threads on that engine, and an error's text goes
 * to srtp_engine_last_error.  n = 0 returns SRTP_OK and launches nothing;
 * SRTP_EINVAL for a NULL engine, key or array or a key_len other than 16 / 32. */
int srtp_aes_gcm_device(srtp_engine *e, int32_t open, const uint8_t *key, int32_t key_len,
                        uint8_t *seg, const uint32_t *off, const uint32_t *aad_len,
                        const uint32_t *len, const uint8_t *iv, uint8_t *tag, int32_t *result,
                        uint32_t n, void *stream);
/* The same with flags (0: srtp_aes_gcm_device itself).  SRTP_GCM_BATCH_WAVE
 * gives each packet a wave instead of a lane (k_gcm_aead_wave, the stateless
 * twin of the engine's k_gcm_wave): GHASH as a sum over the powers H^1..H^64,
 * which then travel in the kernel's arguments too, a block per lane, and the
 * AES-CTR blocks spread over the lanes.  Same arguments, same results to the
 * byte; SRTP_EINVAL for any other flag bit. */
#define SRTP_GCM_BATCH_WAVE 0x1u
int srtp_aes_gcm_device_ex(srtp_engine *e, int32_t open, const uint8_t *key, int32_t key_len,
                           uint8_t *seg, const uint32_t *off, const uint32_t *aad_len,
                           const uint32_t *len, const uint8_t *iv, uint8_t *tag, int32_t *result,
                           uint32_t n, uint32_t flags, void *stream);
/* Host GF(2^128) arithmetic in GCM's bit order, for tests: out = a * b (16-byte
 * blocks as GHASH takes them; SP 800-38D algorithm 1), and out[16 k ..] =
 * h^(k + 1) for k = 0..63, the powers the wave kernels multiply by. */
int srtp_gf128_mul(const uint8_t a[16], const uint8_t b[16], uint8_t out[16]);
int srtp_gcm_hpowers(const uint8_t h[16], uint8_t out[1024]);

/* The stateless geometry of one packet under the AES-GCM profiles (host only;
 * the function the GPU passes take every offset from): the status the lengths
 * alone decide (`status`, -1: none), else the head AAD [0, aad_len), the
 * E|index word's place (word_at, -1: none; word_aad: it is AAD too, behind the
 * head AAD; unprotect reads it there, protect writes it), the data
 * [data_at, data_at + data_len), the tag [tag_at, tag_at + 16) and the length
 * the packet leaves with (new_len; under an early status, the length
 * reported).  A range is handed out only inside [0, cap).  header_len: the RTP
 * header length or SRTP_GCM_HDR_THROW (ignored for SRTCP); e_bit: SRTCP
 * unprotect, the word's E bit (word_at does not depend on it); decipher: 0 for
 * an SRTP unprotect flagged DISCARD / SILENCE.  Stateful checks lie between:
 * ERR_CAPACITY precedes every state change, SRTP's replay check precedes its
 * ERR_MALFORMED / DROP_AUTH, SRTCP's follows them. */
#define SRTP_GCM_HDR_THROW ((int32_t)0x80000000)
typedef struct {
    int32_t status, new_len, aad_len, word_at, word_aad, data_at, data_len, tag_at, decipher;
} srtp_gcm_job;
int srtp_gcm_packet_job(int32_t kind, int32_t reverse, int32_t len, int32_t cap, int32_t header_len,
                        uint32_t flags, int32_t e_bit, srtp_gcm_job *out);
/* The two rules of the one-pass open (host only; gcm_job.h, the text the GPU
 * passes compile).  srtp_gcm_spec_ok: 1 when the pass before the walk may
 * decipher an unprotect packet of this geometry -- its job has no status, it is
 * not flagged DISCARD / SILENCE, it has data, SRTCP: E = 1, SRTP: header_len is
 * at least the fixed header 12 + 4 CC (+ 4 with X) that byte0 announces (a
 * negative extension length can give less, and the bytes the fix pass re-reads
 * would lie inside the deciphered range); else 0; -1 for an unknown kind.
 * srtp_gcm_fix_action: what the pass after the walk owes a packet, from
 * whether it was deciphered before the walk (spec_done), its final status,
 * whether it is to leave deciphered (wanted: status OK, no DISCARD / SILENCE,
 * SRTCP: E = 1) and, for SRTP (rtp), the ROC guess g0 and the walk's ROC cw. */
#define SRTP_GCM_FIX_NONE 0
#define SRTP_GCM_FIX_RESTORE 1  /* the CTR pass again under the speculation's IV: ciphertext back */
#define SRTP_GCM_FIX_DECIPHER 2 /* decipher under the walk's ROC / the index word */
int32_t srtp_gcm_spec_ok(int32_t kind, int32_t len, int32_t cap, int32_t header_len, uint32_t flags,
                         int32_t e_bit, uint32_t byte0);
int32_t srtp_gcm_fix_action(int32_t spec_done, int32_t final_status, int32_t wanted, int32_t rtp, uint32_t g0,
                            uint32_t cw);

/* DTLS-SRTP keying (control plane, host only): what
 * DtlsPacketTransformer.initializeSRTPTransformer does after the handshake
 * (transform/dtls/DtlsPacketTransformer.java:549-690).
 *
 * srtp_tls_export_keying_material is the RFC 5705 exporter the reference calls
 * through BouncyCastle's TlsContext.exportKeyingMaterial(ExporterLabel.dtls_srtp,
 * null, n) (:614-617): PRF(master_secret, label, client_random ||
 * server_random)[0..out_len) with no context value.  prf selects the TLS PRF
 * of the negotiated version: SRTP_TLS_PRF_TLS10 (DTLS 1.0, RFC 2246 5: P_MD5 xor
 * P_SHA1 over the secret's halves -- the version the reference offers,
 * TlsClientImpl.java:148-155) or SRTP_TLS_PRF_SHA256 (DTLS 1.2, RFC 5246 5).
 * The label for DTLS-SRTP is SRTP_DTLS_EXPORTER_LABEL.
 *
 * srtp_dtls_profile_keys fills the policies of a negotiated protection profile
 * (:574-612; the _32 profiles keep a 10-byte SRTCP tag) and splits
 * keying_material_len = 2 * (key + salt) bytes of exported material as client
 * key | server key | client salt | server salt (:618-638).  km == NULL fills
 * only the lengths and policies.  Unknown profile: SRTP_EPOLICY (the
 * reference's IllegalArgumentException).
 *
 * srtp_dtls_transformer_create builds both factories (the client's is a sender
 * iff is_client, the server's iff !is_client: :639-652) and a transformer of
 * `kind` whose forward factory is this side's own and reverse the peer's
 * (:653-690).  NULL-cipher profiles, which export no master key (the
 * reference then fails deriving session keys), return
 * SRTP_EPOLICY.  out_factories (may be NULL) receives {client, server} factory ids
 * -- the caller closes them with the transformer, as
 * SRTPTransformer.close() closes both (SRTPTransformer.java:132-150). */
#define SRTP_PROFILE_AES128_CM_HMAC_SHA1_80 0x0001
#define SRTP_PROFILE_AES128_CM_HMAC_SHA1_32 0x0002
#define SRTP_PROFILE_NULL_HMAC_SHA1_80 0x0005
#define SRTP_PROFILE_NULL_HMAC_SHA1_32 0x0006
/* RFC 7714 14.2 (16- / 32-byte key, 12-byte salt, 16-byte tag).
 * srtp_dtls_profile_keys answers SRTP_EPOLICY for them, as it always has;
 * srtp_dtls_profile_keys_ex with SRTP_DTLS_AEAD knows them: both policies the
 * GCM shape, keying_material_len = 2 * (key + 12), the same client key |
 * server key | client salt | server salt split (RFC 5764 4.2).  Without the
 * flag it is srtp_dtls_profile_keys with wider key fields. */
#define SRTP_PROFILE_AEAD_AES_128_GCM 0x0007
#define SRTP_PROFILE_AEAD_AES_256_GCM 0x0008
#define SRTP_TLS_PRF_TLS10 0
#define SRTP_TLS_PRF_SHA256 1
#define SRTP_DTLS_EXPORTER_LABEL "EXTRACTOR-dtls_srtp"
typedef struct {
    srtp_policy srtp, srtcp;
    int32_t key_len, salt_len, keying_material_len;
    uint8_t client_key[16], server_key[16];
    uint8_t client_salt[14], server_salt[14];
} srtp_dtls_keys;
int srtp_tls_export_keying_material(int32_t prf, const uint8_t *master_secret, int32_t secret_len,
                                    const uint8_t client_random[32], const uint8_t server_random[32],
                                    const char *label, uint8_t *out, int32_t out_len);
int srtp_dtls_profile_keys(int32_t profile, const uint8_t *km, int32_t km_len, srtp_dtls_keys *out);
#define SRTP_DTLS_AEAD 0x1u
typedef struct {
    srtp_policy srtp, srtcp;
    int32_t key_len, salt_len, keying_material_len;
    uint8_t client_key[32], server_key[32];
    uint8_t client_salt[14], server_salt[14];
} srtp_dtls_keys_ex;
int srtp_dtls_profile_keys_ex(int32_t profile, const uint8_t *km, int32_t km_len, srtp_dtls_keys_ex *out,
                              uint32_t flags);
int srtp_dtls_transformer_create(srtp_engine *e, int32_t profile, int32_t is_client, int32_t kind,
                                 const uint8_t *km, int32_t km_len, int32_t *out_transformer,
                                 int32_t out_factories[2]);

#ifdef __cplusplus
}
#endif
#endif
