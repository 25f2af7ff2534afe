/*
 * lamejs_hip.h -- C ABI of the MI355X-native MP3 frame-encode path (liblamejs_hip.so).
 *
 * This is the drop-in boundary for the hot path of zhuker/lamejs: everything that
 * `Mp3Encoder.encodeBuffer()/flush()` does after parameter resolution.  The entry points are
 * what the reference's JavaScript front end would bind through a thin N-API addon
 * (lamejs_amd/js/addon/lhip_napi.c); plain pointers and sizes only.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   lhip_create   <- new Mp3Encoder(channels, samplerate, kbps)      src/js/index.js:66-111
 *                    (lame_init + lame_init_params; the resolved tables arrive as one blob built by
 *                     the host-side JavaScript lamejs_amd/js/tables.js with the host's own Math.*)
 *   lhip_encode   <- Mp3Encoder.encodeBuffer(left, right)            src/js/index.js:117-130
 *                    -> Lame.lame_encode_buffer                      src/js/Lame.js:1490-1514
 *                    -> lame_encode_buffer_sample                    src/js/Lame.js:1527-1667
 *                    -> Encoder.lame_encode_mp3_frame (hot path)     src/js/Encoder.js:388-659
 *   lhip_flush    <- Mp3Encoder.flush() -> Lame.lame_encode_flush    src/js/index.js:132-135, Lame.js:1381-1488
 *   lhip_destroy  <- (garbage collection of the encoder object)
 *
 * Channel mode.  The reference's Mp3Encoder hard-codes MPEGMode.STEREO for two channels (index.js:105).  As an extension the
 * blob may carry mode = 1 (tables.js buildBlob(..., { jointStereo: true })): the stream is then encoded in the reference core's
 * joint-stereo mode -- per frame mid/side or left/right (Encoder.js:520-561) -- byte for byte what the reference's own modules
 * produce when asked for MPEGMode.JOINT_STEREO.  Nothing in the signatures below changes.
 * Bit reservoir.  Likewise disable_reservoir = 0 in the blob ({ reservoir: true }; index.js:108 hard-codes it off): the frames of a
 * stream then depend on each other (budget and masking), so the library encodes one frame per stream per launch -- batches of many
 * streams are what uses the GPU -- the byte count of a call is data-dependent, and every call synchronises (sync = 0 is ignored).
 *
 * Resampling by a non-integer ratio.  By default a configuration whose output rate is not an integer fraction of the input rate is refused
 * (the reference feeds itself NaN samples there once a call is long enough).  A blob built with { fractionalResample: true } carries the
 * reference's set-up for it (filter_l = 31, all 2 * bpc + 1 windows); the stream is then a CALL-SEQUENCE stream: the bytes of every
 * lhip_encode are the reference's for the same sequence of call lengths (they do depend on where the calls are cut -- the reference's do).
 * A call the reference would not consume whole returns -4 and consumes nothing, lhip_last_error() names the length that is always accepted
 * (lhip_frac_call_limit(): 1585 samples for 44100 -> 32000 Hz, never less than 576); each call completes 0 or 1 frame; lhip_encode_output_bytes
 * stays exact (-4 for a call that would be refused).  lhip_flush: the flush frames whose input the reference still computes from whole
 * positions are encoded byte for byte; those in which it encodes its own NaN samples (audibly empty there too) are replaced by silent frames
 * of equal length and header; the stream ends with its flush (a later lhip_encode returns -4).  lhip_seek, lhip_state_get and lhip_state_set
 * return -4 for such streams; the bit reservoir cannot be combined with it.  lhip_encode_batch over such streams may mix configurations.
 *
 * Sample formats.  lhip_encode takes Int16 planes; lhip_encode_pcm and the *_pcm batch entries take Int16 or Float32, planar or interleaved
 * (see LHIP_PCM_* below): Float32 is what the reference itself encodes, so fractional samples and samples beyond 16 bits give its bytes.
 * They also take what a WAV file stores -- 8-bit unsigned, packed 24-bit, 32-bit integers, floats and doubles in [-1, 1] -- and doubles used as
 * given; a kernel of its own (g_ingest) turns those into Float32 planes in front of the call's first reader, so no host-side pass widens them.
 *
 * Input gains and downmix (extension).  A blob built with { downmix, scale, scaleLeft, scaleRight } (tables.js) carries the reference's
 * gfp.scale / scale_left / scale_right and, for a downmix, MPEGMode.MONO with two input channels (Lame.js:1551-1584).  lhip_config.channels
 * counts INPUT channels: a downmix stream is created with channels = 2, takes two-channel calls through every entry below and is a
 * one-channel stream behind the read sites (output sizes, state).  Per sample, in the reference's order, each product an f64 product stored to
 * Float32:  a = l (* scale) (* scale_left);  b = r (* scale, only when two channels go out) (* scale_right);  downmix m = (float)(0.5 * (a + b)).
 * lhip_create returns -3 with a message for a gain that is not finite, a negative scale, or a combined gain of a channel above 4 in
 * magnitude; the Float32 sample limit of such a stream is 131072 / max(1, |gain left|, |gain right|).  lhip_seek applies the same arithmetic
 * to its Int16 tails (a downmix stream needs both).
 *
 * Frame protection and header flags (extension).  A blob built with { protect } (tables.js) carries error_protection = 1 and a sideinfo_len
 * two bytes above the mode's (Lame.js:1109-1110): every frame then holds a CRC-16 as ISO 11172-3 defines it (polynomial 0x8005, preset
 * 0xffff, over header bytes 2, 3 and the side information) in bytes 4, 5, computed by the kernels that format frames.  Frame sizes, and
 * with them lhip_encode_output_bytes and lhip_max_output_bytes, do not change; each frame has 16 bits less for main data.  { copyright,
 * original, privateBit, emphasis } set the header bits of those names.  lhip_create returns -3 with a message when sideinfo_len does not fit
 * the flag, for a flag that is not 0 or 1, for emphasis 2 (reserved), and for error_protection on a non-integer-ratio stream.
 *
 * Info tag (extension).  A blob built with { infoTag } (tables.js) makes the stream a FILE: its first call that returns anything -- the first lhip_encode* with
 * samples, or the flush -- returns, in front of its audio, a placeholder of lhip_stream_info_t::tag_bytes bytes (a valid frame header, then zeros; LAME's
 * contract), written by the host; the audio behind it is byte for byte the stream without the option, and lhip_max_output_bytes / lhip_encode_output_bytes
 * count the placeholder while it is pending.  The library keeps the stream's totals on the host -- frames, audio bytes, a 100-point seek table's bag, delay
 * and end padding -- and the CRC-16 of all audio bytes (the "music CRC": reflected polynomial 0xA001, preset 0), computed where the bytes are: by a kernel
 * behind the call's last writer for bytes that stay in HBM, by the host for a small call whose bytes arrive in pinned memory anyway.  A device-pointer
 * batch with such a stream fetches the CRCs at the end of the call, so it synchronises (sync = 0 is ignored).  After lhip_flush, lhip_info_tag writes the
 * finished tag frame ("Info", frames, bytes, seek table, "LAME3.98r" and LAME's extension fields, music CRC, tag CRC); the caller writes it over the
 * placeholder at offset 0 of the file.  lhip_create returns -3 with a message where the frame (floor((version + 1) * 72000 * brate / out_samplerate)
 * bytes) cannot hold sideinfo_len + 156 bytes, and for a stream that resamples by a non-integer ratio.  State blobs do not carry the totals: lhip_info_tag
 * on a stream moved with lhip_seek or lhip_state_set returns -4.
 *
 * Output sample rate and filters (extension).  A blob built with { outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth } (tables.js) carries the
 * reference core's gfp.out_samplerate, lowpassfreq, lowpasswidth, highpassfreq and highpasswidth as it carries the automatic choice: in out_samplerate,
 * version, mode_gr, brate, the resampler tables and the 32 band factors of amp_filter (Lame.js:470-558, the highpass half included).  No entry and no
 * configuration field is added.  lhip_create returns -3 with a message for an amp_filter value that is not finite or lies outside [0, 1].
 *
 * Semantics preserved: any chunking of the same sample stream yields the same bytes; a call
 * returns the bytes of all whole frames completed by that call (possibly 0); errors are negative
 * return codes mirroring the reference (-1 output buffer too small, -3 bad handle, -4 internal/device
 * error).  A stream handle is not thread-safe (same as the reference); distinct handles are independent.
 * The library never retains caller pointers past the call.
 *
 * There is NO CPU fallback: if no HIP device is usable every entry point fails with -4 and
 * lhip_last_error() explains why.
 */
#ifndef LAMEJS_HIP_H
#define LAMEJS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lhip_stream lhip_stream;

typedef struct lhip_config {
    int32_t channels;     /* 1 or 2 (as passed to Mp3Encoder): INPUT channels -- 2 for a downmix blob */
    int32_t samplerate;   /* Hz */
    int32_t kbps;         /* CBR bitrate */
    int32_t device;       /* HIP device ordinal; -1 = current device */
} lhip_config;

#define LHIP_ERR_BUFFER_TOO_SMALL (-1)
#define LHIP_ERR_BAD_HANDLE       (-3)
#define LHIP_ERR_INTERNAL         (-4)

/* number of usable HIP devices (0 if none / runtime unavailable) */
int lhip_device_count(void);

/* Restrict the devices the library may place streams on: bit d of `mask` = HIP device d.  A later
 * lhip_create with cfg.device == -1 then deals streams round-robin over the allowed devices (independent streams are the
 * path's multi-GPU axis); an explicit cfg.device outside the mask is refused.  mask == 0 restores the default (every
 * device; device -1 = the calling thread's current HIP device).  Returns the number of allowed devices or <0. */
int lhip_set_devices(uint64_t mask);
/* the HIP device a stream was placed on (>= 0), or LHIP_ERR_BAD_HANDLE */
int lhip_stream_device(const lhip_stream* s);
/* What tells two GPUs apart: PCI bus id ("0000:a7:00.0") and UUID (32 hex digits) of HIP device `device` (-1 = current), as NUL-terminated strings of at most
 * `cap` bytes each (40 is enough).  bench.py prints them per rank, so that a multi-GPU line shows N ranks on N distinct devices.  Returns 0 or <0. */
int lhip_device_identity(int device, char* pci_bus_id, char* uuid_hex, size_t cap);

/* Frame-range sharding of ONE stream (extension; SURVEY.md 8e, second mode).  A long stream can be cut at frame boundaries and the
 * pieces encoded side by side (other GPUs, other processes): the state at a cut is SPECULATED -- lhip_seek puts a fresh stream at an
 * input position with the samples in front of it, a few warm-up frames (output discarded) let the masking history, the
 * filterbank overlap, the attack / block-type chains, the ATH adjustment and the bin-search seeds converge -- and then VERIFIED:
 * lhip_state_get of that stream at the cut must equal, byte for byte, lhip_state_get of the stream that encoded up to the cut; if it
 * does, everything after the cut is what one stream would have produced (64 warm-up frames verified at every cut of every stream tried,
 * material with long silences included; 8 are enough on steady material).  On a miss the true state is transplanted (lhip_state_set)
 * and the piece is encoded again.  bench.py --config shard3 does exactly that over torch.distributed
 * (one range per rank; tests/test_shard_gloo.py runs it with two and three ranks, tests/test_hostsim_parity.py the API itself).
 *   lhip_seek(s, sample_pos, tail_l, tail_r): s fresh; sample_pos a whole number (>= 2) of frames; tail_*: the lhip_seek_tail_samples(s)
 *   input samples in front of sample_pos (host memory).  Not for resampling or bit-reservoir streams. */
/* lhip_state_get returns the blob in canonical form (fields no later launch can read are zeroed), so two streams that stand at the
 * same point compare equal whatever call sizes took them there.  lhip_state_set may be applied to a fresh or to a used stream of the
 * same configuration (it replaces everything the stream carries); like every call on a handle it must not run concurrently with
 * another call on the same handle.  A two-channel lhip_seek needs both tails. */
size_t lhip_state_bytes(const lhip_stream* s);
int lhip_state_get(lhip_stream* s, void* buf, size_t cap);
int lhip_state_set(lhip_stream* s, const void* buf, size_t n);
size_t lhip_seek_tail_samples(const lhip_stream* s);
int lhip_seek(lhip_stream* s, int64_t sample_pos, const int16_t* tail_left, const int16_t* tail_right);

/* Create an encoder stream.  `tables` is the LHTB blob produced by lamejs_amd/js/tables.js for
 * (channels, samplerate, kbps); it is validated against cfg, uploaded to HBM (shared between
 * streams with identical blobs) and may be freed by the caller on return.  Returns 0 or <0. */
int lhip_create(const lhip_config* cfg, const void* tables, size_t tables_bytes, lhip_stream** out);

/* Append nsamples Int16 samples per channel (right may be NULL for mono) and write the bytes of
 * every MP3 frame completed by them to out.  Returns bytes written (>= 0) or a negative code. */
int64_t lhip_encode(lhip_stream* s, const int16_t* left, const int16_t* right, size_t nsamples,
                    uint8_t* out, size_t out_cap);

/* Sample formats (extension).  The reference's encodeBuffer stores whatever numbers it is given into a Float32Array and encodes those
 * (Lame.js:1506-1510); PCM on disk and on the wire is interleaved.  A format is a sample type, LHIP_PCM_S16 or LHIP_PCM_F32, optionally
 * or-ed with LHIP_PCM_INTERLEAVED; one format per call, any format at any call of a stream.  The *_pcm entries below are the entries
 * above them with a format: the old entries ARE their LHIP_PCM_S16 planar case.
 *   F32: the sample is used as the Float32 it is (then `gfp.scale` where it applies: (float)((double)v * scale), as for Int16).  For
 *        integer values inside the Int16 range the bytes are those of the Int16 call.
 *   INTERLEAVED: left points at channels * nsamples samples (L R L R ...), right is ignored; byte for byte the result of the planar call
 *        on the de-interleaved samples.  For a one-channel stream interleaved is planar.  nsamples always counts samples per channel.
 * The one deviation from the reference: every F32 sample must be finite with |x| <= 131072.0 (four times Int16 full scale).  The
 * reference encodes NaN and infinities into garbage; here they never reach a kernel.  Host-pointer entries look at the whole call first:
 * a bad sample gives -4, lhip_last_error() names stream, channel, index and value, and nothing is consumed on any stream.  The
 * device-pointer entry cannot see the values: every read site reads such a sample as 0.0f, and lhip_last_batch_rejected_samples()
 * reports how many (stream, channel, sample) positions of the calling thread's last batch were read that way (it synchronises).
 * lhip_seek keeps its Int16 tails; state blobs do not depend on the formats that produced them. */
#define LHIP_PCM_S16         0
#define LHIP_PCM_F32         1
#define LHIP_PCM_INTERLEAVED 2
/* Sample types of WAV files (extension).  The sample type of a format is `format & ~LHIP_PCM_INTERLEAVED`; INTERLEAVED may be or-ed to each.  A type is
 * defined by the number the reference would find in its Float32 buffer had the caller widened the samples for it:
 *   U8    1 byte, unsigned                          (b - 128) * 256, exact
 *   S24   3 bytes, little-endian, packed            v / 256, exact in Float32; any address
 *   S32   int32                                     (float)(v / 65536.0): one rounding, to nearest even
 *   F32N  float in [-1, 1]                          x * 32768
 *   F64N  double in [-1, 1]                         (float)(x * 32768.0): one rounding
 *   F64   double, used as given                     (float)x: what a Float64Array handed to the reference becomes
 * The Float32 contract follows the conversion: the value must be finite with |v| <= the stream's limit (131072, less where its gains exceed 1); F64N and
 * F64 are compared before their rounding, so a double above the limit is refused even where it would round onto it.  Host-pointer entries refuse such a
 * call with -4 (stream, channel, index and value in lhip_last_error()) and consume nothing; the device-pointer entry reads such a sample as 0.0f and counts
 * it in lhip_last_batch_rejected_samples().  Integer types cannot leave the contract and are never scanned.  Device pointers of the 4- and 8-byte types
 * among these must be multiples of the element size (-4 with a message otherwise); U8 and S24 may lie at any address.  A format whose type is none of the
 * values defined here returns -4.  A stream may change type from call to call; state blobs, lhip_seek's Int16 tails and the output-size entries do not
 * depend on the type.  A call in one of these types is converted once into Float32 planes of the device context (the kernel g_ingest, LHIP_PATH_INGEST;
 * a host call small enough for one pinned block is converted by the host while it fills that block) and is a Float32 planar call from there on. */
#define LHIP_PCM_U8          4
#define LHIP_PCM_S24         8
#define LHIP_PCM_S32         12
#define LHIP_PCM_F32N        16
#define LHIP_PCM_F64N        20
#define LHIP_PCM_F64         24
int64_t lhip_encode_pcm(lhip_stream* s, int format, const void* left, const void* right, size_t nsamples,
                        uint8_t* out, size_t out_cap);

/* Pad with zeros until all buffered samples are emitted (reference flush rules); a second call
 * returns 0. */
int64_t lhip_flush(lhip_stream* s, uint8_t* out, size_t out_cap);

void lhip_destroy(lhip_stream* s);

/* Upper bound of the bytes lhip_encode can return for nsamples more samples on this stream. */
size_t lhip_max_output_bytes(const lhip_stream* s, size_t nsamples);

/* Exactly the bytes the next lhip_encode(s, ..., nsamples, ...) will return: under CBR without the bit reservoir the frame sizes follow
 * from the sample count and the padding accumulator alone, so a binding can allocate the returned array at its final size and let the
 * library write into it -- no second buffer, no copy (the reference allocates a fresh exact-size Int8Array per call, index.js:129).
 * With the bit reservoir (extension) the count is data-dependent and this returns lhip_max_output_bytes().  < 0: bad handle. */
int64_t lhip_encode_output_bytes(const lhip_stream* s, size_t nsamples);
/* 1: lhip_encode_output_bytes(s, n) is the exact byte count of the next call (CBR without the bit reservoir); 0: it is only an upper bound (bit-reservoir
 * extension: the count is data-dependent) -- a binding then encodes into scratch memory and hands out an exact copy; < 0: bad handle. */
int lhip_output_bytes_is_exact(const lhip_stream* s);

/* Batch extension (BASELINE config 5: many independent streams, one launch): stream i receives
 * nsamples[i] samples from left[i]/right[i] and its frames are written to out[i] (capacity
 * out_cap[i]); written[i] receives the byte count or a negative code.  All streams must share one
 * device.  Streams of one configuration (same tables blob) share a launch; a batch that mixes table blobs --
 * protected beside unprotected streams, say -- is launched blob by blob in order of first appearance and
 * synchronises; a refusal in a later group leaves the earlier groups encoded (written[] says which).
 * Returns 0 or the first negative code. */
int lhip_encode_batch(lhip_stream* const* streams, size_t nstreams, const int16_t* const* left,
                      const int16_t* const* right, const size_t* nsamples, uint8_t* const* out,
                      const size_t* out_cap, int64_t* written);
int lhip_encode_batch_pcm(lhip_stream* const* streams, size_t nstreams, int format, const void* const* left,
                          const void* const* right, const size_t* nsamples, uint8_t* const* out,
                          const size_t* out_cap, int64_t* written);
int lhip_flush_batch(lhip_stream* const* streams, size_t nstreams, uint8_t* const* out,
                     const size_t* out_cap, int64_t* written);

/* Device-resident variants: the pointers are HBM addresses on the stream's device (e.g. a
 * torch tensor's data_ptr()); nothing crosses PCIe except a few hundred bytes of descriptors.
 * Work is enqueued on the HIP stream set by lhip_set_hip_stream (default: the null stream) and the
 * call returns after enqueueing unless `sync` is non-zero: nothing in the pipeline waits for the host (the bin-search seed chain
 * is validated and repaired by a persistent kernel on the device), so with sync == 0 the output bytes and lhip_last_batch_stats
 * are only valid after the stream has been synchronised (lhip_last_batch_stats does that itself).  The input buffers are read by
 * kernels up to the end of the batch (the samples are converted where they are consumed, there is no staging copy), so with
 * sync == 0 they must stay valid and unchanged until then as well. */
int lhip_encode_batch_device(lhip_stream* const* streams, size_t nstreams, const int16_t* const* d_left,
                             const int16_t* const* d_right, const size_t* nsamples, uint8_t* const* d_out,
                             const size_t* out_cap, int64_t* written, int sync);

int lhip_encode_batch_device_pcm(lhip_stream* const* streams, size_t nstreams, int format, const void* const* d_left,
                                 const void* const* d_right, const size_t* nsamples, uint8_t* const* d_out,
                                 const size_t* out_cap, int64_t* written, int sync);
/* F32 samples outside the contract that the last lhip_encode_batch_device_pcm of the calling thread read as zero (0 after any other call);
 * waits for that batch.  A two-channel planar call whose right plane is NULL or the left plane counts each sample once.  The counter lives with the
 * device context: fetch it before another thread starts a Float32 device batch on the same device (a handle is not thread-safe, and neither
 * is this pairing of a batch with its count).  < 0: device error. */
int64_t lhip_last_batch_rejected_samples(void);

/* Use this hipStream_t (passed as void*) for all work of streams on `device` (-1 = current). */
int lhip_set_hip_stream(int device, void* hip_stream);

/* Statistics of the most recent batch on the calling thread: frames encoded, frames that needed
 * the bin-search seed repair pass, repair iterations. */
void lhip_last_batch_stats(int64_t* frames, int64_t* repaired_frames, int64_t* repair_iterations);

/* Debug/test hook: which launch paths the most recent batch on the calling thread took -- a host-side record of the decisions the library
 * made from the batch's shape and the device's CU count (no kernel is changed or synchronised for it); a long host call that was cut into
 * units reports every path one of its units took.  One bit per decision:
 *   LHIP_PATH_FRAME 0x1 (the one-launch frame program, g_frame<0>), FRAME_RESV 0x2 (g_frame<1>, bit reservoir), SEPARATE 0x4 (the separate
 *   kernels), PREP 0x8 (the resampler materialises samples), PSY4 0x10 (joint stereo's second analysis launch), QUANT_PAIR 0x20 (g_quant_pair),
 *   QUANT_PERSISTENT 0x40 (g_quant, for two channels with the tail help), RESV_STREAM_HELPERS 0x80 / RESV_STREAM_NOHELPERS 0x100 (g_resv_stream
 *   with / without its count helpers), RESV_FLUSH 0x200 (g_resv_flush behind the frame program), FIXUP_SINGLE 0x400 / FIXUP_COOP 0x800 (g_fixup as
 *   one workgroup / as a cooperative launch), SMALL_CALL 0x1000 (everything in one pinned block).
 * Returns 0, or < 0 for a null pointer. */
#define LHIP_PATH_FRAME 0x1u
#define LHIP_PATH_FRAME_RESV 0x2u
#define LHIP_PATH_SEPARATE 0x4u
#define LHIP_PATH_PREP 0x8u
#define LHIP_PATH_PSY4 0x10u
#define LHIP_PATH_QUANT_PAIR 0x20u
#define LHIP_PATH_QUANT_PERSISTENT 0x40u
#define LHIP_PATH_RESV_STREAM_HELPERS 0x80u
#define LHIP_PATH_RESV_STREAM_NOHELPERS 0x100u
#define LHIP_PATH_RESV_FLUSH 0x200u
#define LHIP_PATH_FIXUP_SINGLE 0x400u
#define LHIP_PATH_FIXUP_COOP 0x800u
#define LHIP_PATH_SMALL_CALL 0x1000u
/* (one more bit, stated as a shift: OUT_CRC 0x2000 -- the batch held { infoTag } streams and their music CRC was computed by the kernel g_out_crc; such a
 *  batch without this bit took the host's CRC over the pinned mirror of a SMALL_CALL) */
#define LHIP_PATH_OUT_CRC (1u << 13)
/* (and INGEST 0x4000: samples of a LHIP_PCM_U8 .. LHIP_PCM_F64 call were turned into Float32 planes by the kernel g_ingest; such a call without this bit was a
 *  SMALL_CALL, converted by the host) */
#define LHIP_PATH_INGEST (1u << 14)
/* (and GAIN 0x8000: the batch held { replayGain } streams: the kernels g_gain_stage and g_gain ran behind it; never set for a stream without the option) */
#define LHIP_PATH_GAIN (1u << 15)
/* (and QUANT_FAST 0x10000: the batch's streams were built with { quality: 7 } and its speculative quantization pass was the bin-search-only kernel g_quant_fast
 *  instead of QUANT_PAIR / QUANT_PERSISTENT; never set for reservoir streams, one-frame calls or with LAMEJS_HIP_NO_FAST_QUANT=1 in the environment) */
#define LHIP_PATH_QUANT_FAST (1u << 16)
int lhip_debug_last_paths(uint32_t* mask);

/* Info tag (extension; see above).  What a stream built with { infoTag } has put out so far, and the finished tag frame. */
typedef struct lhip_stream_info_t {
    int64_t frames;        /* audio frames encoded */
    int64_t audio_bytes;   /* audio bytes returned (the placeholder is not among them) */
    uint32_t music_crc;    /* CRC-16 of those bytes */
    int32_t delay;         /* encoder delay in samples (576) */
    int32_t padding;       /* samples of padding at the end of the stream; -1 before the flush */
    int32_t tag_bytes;     /* size of the tag frame = of the placeholder */
} lhip_stream_info_t;
/* 0, or < 0 with a message (-4: the stream was not built with the option) */
int lhip_stream_info(const lhip_stream* s, lhip_stream_info_t* info);
/* Valid after the flush: writes the tag frame to out (capacity cap) and returns its size; -1: cap too small; -4 with a message: not flushed yet, not a
 * tagged stream, or a stream that was moved with the seek / state entries. */
int64_t lhip_info_tag(lhip_stream* s, uint8_t* out, size_t cap);
/* Test hooks.  lhip_debug_crc_span: the bytes one workgroup of the CRC kernel covers.  lhip_debug_crc16: THE KERNEL (in the simulation libraries: its body) over
 * n bytes of the caller's, placed misalign (0 .. 15) bytes past a 16-byte boundary of device memory -- always the device path, whatever n is; *crc receives
 * the CRC-16.  lhip_debug_info_toc: the seek table's bookkeeping alone -- ncalls batches of frames[i] frames of kbps each, then the 100 seek points into toc;
 * returns the number of bag entries in use or < 0. */
size_t lhip_debug_crc_span(void);
int lhip_debug_crc16(const void* bytes, size_t n, size_t misalign, uint32_t* crc);
int lhip_debug_info_toc(const int64_t* frames, size_t ncalls, int kbps, uint8_t* toc);
/* ReplayGain (extension): a stream whose table blob was built with { replayGain } analyses the Float32 samples its encoder consumes -- behind the input gains,
 * the downmix and the resampler; every call's new samples, the zeros of the flush included; the left and right channel of a joint-stereo stream -- on the
 * device, by the published ReplayGain method as the reference's GainAnalysis.js states it: per output channel a 10th-order "Yule" filter and a 2nd-order
 * Butterworth high-pass (f64 arithmetic, outputs stored as Float32), the energy over windows of ceil(out_samplerate / 20) samples, one count per window in a
 * histogram of 0.01 dB steps; at the end the bin below which 95 % of the windows lie gives the track gain 64.82 dB - bin / 100.
 * The result is a pure function of the sample stream: any cut into calls, encode_batch and the device entries give the same histogram.  A window's energy is
 * computed from a recursion restarted a fixed number of samples in front of it, so it is the reference's bit for bit for the first windows of a stream and
 * within rounding noise (far below one histogram step) elsewhere -- INTEGRATION.md "ReplayGain".  Nothing is read back per call: an asynchronous device call
 * stays asynchronous.  With { infoTag } the tag frame's radio ReplayGain field carries the value (peak amplitude and the audiophile field stay zero).
 * lhip_create returns -3 for a { replayGain } blob that resamples by a non-integer ratio.  State blobs do not carry the analysis.
 * lhip_replay_gain synchronises the stream's device context and returns 0 with *tenth_db = the track gain in tenths of a dB (RadioGain of the reference),
 * *windows = complete windows analysed and *samples = samples analysed; 1 with *tenth_db = 0 when no window is complete yet (the reference asserts there);
 * -4 with a message for a stream without the option or one that was moved with lhip_seek / lhip_state_set. */
int lhip_replay_gain(lhip_stream* s, int32_t* tenth_db, int64_t* windows, int64_t* samples);

/* Quality (extension): a table blob built with { quality: 7 } (tables.js; 8 is resolved to 7) carries the switches of the reference core's fast mode, LAME's
 * -f (Lame.js:577-588): noise_shaping, noise_shaping_amp, noise_shaping_stop and use_best_huffman 0, subblock_gain -1.  The psychoacoustic model still
 * decides block switching and mid/side; the quantization of a granule is the bin search for its step size alone (Quantize.js:886-888).  There is no new
 * entry and no changed record: lhip_create derives one host flag per table set from noise_shaping == 0 && use_best_huffman == 0, and a batch of such
 * streams without the bit reservoir runs its speculative quantization pass in the kernel g_quant_fast (LHIP_PATH_QUANT_FAST) -- one wave per channel, the bin
 * search and nothing else; validation, repair and bit packing behind it are the kernels every stream uses.  One-frame calls, reservoir streams and the repair
 * pass keep the general program, which reads the same switches.  LAMEJS_HIP_NO_FAST_QUANT=1 in the environment (read once per process) sends such batches
 * through the general quantization kernels as well: the same bytes.  LAMEJS_HIP_QUANT_GRID_MAX=<n>, n >= 1 (a test hook, read once per process) launches the
 * persistent speculative quantization kernels, g_quant_fast and g_quant, with at most n workgroups -- with 1, every wave or pair of waves of the one workgroup
 * takes frame after frame -- and touches no other kernel's grid; unset or < 1 it changes nothing.  lhip_debug_read(11) reports the launch.  State blobs, lhip_state_bytes, lhip_seek and every other option work as at quality 3;
 * with { infoTag } the tag reports quality 53 and no noise shaping.  Other quality levels are not in the envelope (tables.js refuses them). */
/* Test hooks.  lhip_debug_gain_histogram: the stream's 12000 histogram counts (synchronises; same refusals).  lhip_debug_gain_windows: THE KERNELS g_gain_stage and
 * g_gain (in the simulation libraries: their bodies) over n samples per channel (l; r for two channels) as one call of a fresh stream at output rate fs: bins and
 * energies receive floor(n / window) entries, each window's histogram bin and its lsum + rsum.  Returns that number of windows, or < 0. */
int lhip_debug_gain_histogram(lhip_stream* s, uint32_t* A);
int lhip_debug_gain_windows(int fs, int channels, const float* l, const float* r, size_t n, int32_t* bins, double* energies);
/* Test hook.  lhip_debug_ingest: THE KERNEL g_ingest (in the simulation libraries: its body) over the caller's samples in `format` (one of the LHIP_PCM_U8 ..
 * LHIP_PCM_F64 types, optionally INTERLEAVED), placed misalign (0 .. 15) bytes past a 16-byte boundary of a device buffer of exactly that size: channels (1 or
 * 2) * nsamples elements -- interleaved, or the left plane followed by the right one.  left / right (right: two channels only) receive nsamples floats each,
 * *rejected the samples read as zero (limit 131072).  misalign must be a multiple of the element size for the 4- and 8-byte types.  Returns 0 or < 0. */
int lhip_debug_ingest(int format, int channels, const void* bytes, size_t nsamples, size_t misalign, float* left, float* right, int64_t* rejected);
/* Test hook.  lhip_debug_quant_probe: THE KERNEL g_quant_probe (in the simulation libraries: its body) over n records `in`, results to the n records `out`, with
 * the tables of stream s.  The kernel calls the quantization search's own device functions -- q_ath_pseudo, q_init_outer_loop, q_init_xrpow, q_calc_xmin,
 * q_pecalc, q_count_bits with the full and with the short round count, q_calc_noise_ -- and restates none.  It reads and writes nothing of the stream's state.
 * One wave per workgroup; a wave takes record after record, so its LDS record serves one record after the other.  max_workgroups: 0 the default grid, 1 every
 * record through one wave, k at most k workgroups (the simulations run at most 3 waves).  Refused (< 0, lhip_last_error says why): null arguments, n = 0 or
 * above 2^20, a quality 7 stream (its table set never calls calc_noise), and any record with a block_type outside 0..3, a global_gain outside 0..255,
 * scalefac_scale or preflag outside 0..1, preflag on a short block, a subblock_gain outside 0..7 (or non-zero on another block type), a scalefac outside 0..255,
 * a band step outside the pow20 table (-116 .. 257) in one of the scalefactor states below, an ix_in outside 0..8206, an unknown flag, or an xr, ratio or
 * ath_adjust that is not finite (ratio >= 0, ath_adjust > 0).  Little-endian, natural alignment, no padding but the named fields.
 * Record in, 4144 bytes:   f32 xr[576] (natural order, as lhip_debug_read(0) gives it; the probe applies the analog-silence rule) | f32 ratio[122] (the E layout
 *   of lhip_debug_read(2)) | f64 ath_adjust | i32 block_type, global_gain, scalefac_scale, preflag, subblock_gain[3], scalefac[39], flags (bit 0: ix_in is
 *   given), pad | i16 ix_in[576] (magnitudes, quantizer line order).
 * Record out, 6352 bytes (zero where a step did not run or does not write):   f64 xrpow_max, pe | i32 active, max_nonzero_coeff, tail0, pad | f32 xr[576] (after
 *   the silence rule, quantizer line order) | f32 xmin[40] | 2 evaluations | 8 calc_noise calls.
 *   An evaluation, 1192 bytes:  i32 bits, big_values, count1, count1table_select, table_select[3], region0_count, region1_count, ran | i16 ix[576].
 *   A calc_noise call, 184 bytes:  f64 max_noise | i32 over_count, over_SSD, ran, pad | f32 distort[40].
 * Steps.  1: q_init_outer_loop, q_init_xrpow -> active, xrpow_max, xr; an inactive record ends here.  2: q_calc_xmin (want_tail0) -> xmin, max_nonzero_coeff,
 * tail0; q_pecalc of ratio with the block type's masking_lower -> pe.  3: one evaluation at global_gain with all scalefactors zero and no noise cache (the bin
 * search's state): q_count_bits with the full round count -> evaluation 0; where tail0 is set, also with the short round count -> evaluation 1, after the
 * words 256..287 of the wave's working spectrum were filled with a pattern and zeroed as the search's caller zeroes them.  A refused gain (bits = 100000)
 * writes bits and ran only.  4: calc_noise with the record's global_gain, scalefac_scale, preflag, subblock_gain and scalefac on ix_in (flag) or on the lines
 * of step 3 (all zero where the gain was refused) -- a: no cache, max_noise wanted; b: no cache, not wanted; c: fills an empty cache, not wanted; d: the same
 * again (every band cached), wanted; e: scalefac[0] ^= 1 (band 0 alone is fresh), not wanted; f: then scalefac[sfb] ^= 1 for every sfb % 3 == 0 below psymax,
 * wanted; g: then scalefac[b] ^= 1 for b the highest band that ends at or below line 192 (it alone is fresh: the border of the 3-line body), not wanted; h: then
 * scalefac[b + 1] ^= 1 (the band above alone), wanted.  c-h run only where lines exist (ix_in given, or the gain not refused).  max_noise is 0 where calc_noise did not form it (not wanted and
 * over_count > 0).  Returns 0 or < 0. */
int lhip_debug_quant_probe(lhip_stream* s, const void* in, size_t n, void* out, int max_workgroups);
/* Test hook.  lhip_debug_bits_probe: THE KERNEL g_bits_probe (in the simulation libraries: the same bodies) -- the bitstream formatter over n frames `in`, results to
 * the n records `out`, with the tables of stream s (any option set: protect, header flags, joint, a downmix's one output channel).  The kernel calls the packers the
 * library launches, kb_bits and kb_bits_mw, and restates nothing of them.  It reads and writes nothing of the stream's state.  Record k is frame k of a fresh
 * stream: its padding bit comes from the stream's own rule (the slot lag a fresh stream starts with), its place in the output from the packer's closed form.
 * form 0: kb_bits, one wave per workgroup; a wave takes frame after frame through one LDS image.  form 1: kb_bits_mw on GR * C waves of one workgroup, which
 * pack the granule-channels side by side into wave 0's image and meet on two LDS counters, as the one-frame program's last phase does; each wave starts at the
 * bit position the side records announce.  max_workgroups: 0 the default grid, 1 every record through one workgroup, k at most k workgroups (the simulations
 * run at most 3).  GR = 2 for MPEG-1, 1 for MPEG-2 / 2.5; C = the stream's output channels.  Little-endian, natural alignment.
 * Record in, GR * C * 1616 bytes:   GR * C side records in (granule, channel) order, then i16 l3[GR * C][576], the signed quantized lines.  A side record, 464
 *   bytes, is the library's own (lhip_debug_read(4)), 116 i32: part2_3_length, part2_length, big_values, count1, global_gain, scalefac_compress, block_type,
 *   table_select[3], subblock_gain[3], region0_count, region1_count, preflag, scalefac_scale, count1table_select, sfbmax, sfbdivide, 5 words the packer does
 *   not read, scfsi (read from granule 1's records: bit i = band i), scalefac[39] (-1: a band shared through scfsi, granule 1 only; MPEG-2: the partitions' entries
 *   in order, a negative one is written as 0), 50 words the packer does not read, mode_ext (read from the first record, joint stereo only).
 * Record out, 1464 bytes:   u8 bytes[1448] (the frame, zero behind it) | i32 nbytes | i32 status (0; -1: no frame found where the packer could have placed it;
 *   -2: bytes written behind the frame's end) | i64 offset, where in its stream's output the packer placed the frame (read off the output buffer: each record has
 *   a zeroed window of its own there).
 * Refused (< 0, lhip_last_error names the record, the granule-channel and the field) before anything is launched: null arguments, n = 0 or above 8192, a form
 * other than 0 and 1, a bit reservoir stream, and any record with big_values odd or above 576; count1 outside big_values..576 or count1 - big_values not a
 * multiple of 4; a table_select that names no table (4, above 31; 14 is written as 16); |l3| above the largest value of its region's table (15 + 2^linbits - 1
 * with linbits, 0 under table 0) or above 8206; a non-zero line at or above count1; a line above 1 in the count1 region; region0_count above 15, region1_count
 * above 7 (a normal block's: a start / stop block's counts are not transmitted) or their sum past the 22 long bands; sfbmax above 39; sfbdivide above sfbmax; scalefac_compress above 15 (MPEG-2: above 399, or outside 500..511
 * with preflag); scfsi above 15; block_type, global_gain, subblock_gain, preflag, scalefac_scale, count1table_select or mode_ext outside their fields; a
 * scalefactor that does not fit its slen (or -1 outside granule 1); part2_length + part2_3_length above 4095 or different from the bits the record will occupy
 * (kb_bits_mw takes the announced value on trust); a frame whose side information and parts exceed the frame's bits.  Returns 0 or < 0. */
int lhip_debug_bits_probe(lhip_stream* s, const void* in, size_t n, void* out, int form, int max_workgroups);

/* Debug/test taps (tests only): copy intermediate results of the most recent batch to the host.
 * what: 0 xr [granule][ch][576] f32, 1 blocktype [granule][ch] i32, 2 E [granule][psy ch][122] f32 (psy ch = ch, or L R mid side in joint stereo; thresholds
 * handed to the quantizer for that granule: en.l 22, en.s 39, thm.l 22, thm.s 39.  In a lazy batch -- no bit reservoir, on the separate kernels, at least
 * LAMEJS_PSY_LAZY_MIN_FRAMES frame slots (a test hook read per batch; unset: 6 x the device's CUs, never below 1024; 0: always, a huge value: never) -- the
 * en.s / thm.s entries of a psy call are computed only where they are read (a channel of the next granule slot is a short block, or the call is its stream's
 * last of the batch and goes into the stream state) and read zero elsewhere; every smaller batch holds all 122 entries of every call), 3 ath_adjust [frame] f64, 4 side records (struct GrSide); simulation libraries only: 10 two i64, the
 * evaluations of the quantization search this process has made without / with the last round of pairs (lines 512..575 all zero / not); 12 three i64, the calc_noise calls this process has made with 7 / with 9 / with 3
 * spectrum lines per lane (counted by the 64-lane simulation; the one-lane simulation reports zeros).
 * 11 (every library; needs no batch to have run): eight i32, the speculative quantization launch of the calling thread's most recent batch -- [0] workgroups
 * launched, [1] waves per workgroup, [2] frame slots, [3] the kernel (1 g_quant_fast, 2 g_quant_pair, 3 g_quant), [4] [5] its PAIR and SKIP template arguments
 * (g_quant_pair: PAIR 1, g_quant: 0), [6] [7] zero; all zero when the batch launched none (one-frame program, bit reservoir).  The wave simulation reports the
 * one 8-wave workgroup it runs (the pair program: a two-wave workgroup per frame slot), the scalar simulation its three striding waves as one workgroup of 3;
 * both run the SKIP = 1 bodies and report in [5] the form the device launches for the table set.
 * Returns bytes copied or <0. */
int64_t lhip_debug_read(int what, void* dst, size_t cap);

/* Per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the roofline
 * line).  lhip_kernel_timing(1) resets and enables, returns the number of kernels; lhip_kernel_times(i)
 * reports name / accumulated milliseconds / launches of kernel i. */
int lhip_kernel_timing(int enable);
int lhip_kernel_times(int idx, const char** name, double* total_ms, int64_t* launches);

/* Test hook: evaluate the device math used by the path on n doubles.  op: 0 log10, 1 pow(10,x), 2 sqrt,
 * 3 1/x, 4 (double)(float)x, 5 ToInt32, 6 x/3 + x*0.1 (must not fuse), 7 log10 by the branch-free variant for positive
 * normal operands / +inf / NaN, 8 the quantizer's two truncations on records of 21 doubles [istep, xa[5], xb[5], adj_a[5], adj_b[5]]
 * (f32 values) -> [0, floor(x istep) x 10, floor(x istep + adj) x 10], 9 calc_noise's logarithm-free band class: noise_class(x)
 * + 1000 * class from the f64 log10 + 1e6 * class from its Float32 copy (the first must equal both others unless it is -1), 10 calc_noise's
 * division by a Float32 through its reciprocal on records of 2 doubles [a, b] -> [div_by_f32(a, (float)b), a / (float)b] (must be equal bit for bit),
 * 11 mask_add's table index for x >= 1: ma_index16(x) (-1 = take the logarithm) + 1000 * ToInt32(log10(x) * 16). */
int lhip_debug_math(int op, const double* in, double* out, size_t n);

/* Test hook: the seed the speculative quantization pass assumes for the reference's bin-search chain
 * (gfc.OldValue / gfc.CurrentStep, Quantize.js:324-326); default 180 / 4.  A poor seed (e.g. 255 / 1) makes the
 * validation flag frames, which exercises the repair passes; the output must not change. */
int lhip_debug_set_spec_seed(int start, int step);

/* Test hook: with LHIP_ALIAS_DEVICES=n in the environment (2 <= n <= 8) the library presents n devices that are n SEPARATE contexts -- own mutex, own HIP
 * stream, own workspaces, own table uploads -- on physical device 0, so that the multi-device paths (lhip_set_devices' round-robin, host threads batching on
 * two contexts at once) run against real HIP on a box with one GPU.  lhip_debug_release_context(d) gives back the stream the library created for such a
 * context (and the side stream of its ATH scan) once no stream lives on it; returns 0 or <0. */
int lhip_debug_release_context(int device);

/* Non-integer-ratio streams (blob built with { fractionalResample: true }): the call length that is accepted whatever calls came before
 * (0 for every other stream: any length goes); < 0: bad handle. */
int64_t lhip_frac_call_limit(const lhip_stream* s);
/* Test hooks for such streams -- the host arithmetic alone, nothing is encoded or consumed.  lhip_debug_frac_call: the output-rate samples (*k)
 * and frames (*frames: 0, 1, or -1 with return code -4 for a call that would be refused) the next lhip_encode of nsamples would make.
 * lhip_debug_frac_flush: what lhip_flush would emit now: returns the number of frames, fills bytes[i] and clean[i] (1: encoded from finite
 * samples, byte-exact; 0: a silent stand-in for a frame the reference makes of NaN samples) for the first `cap` of them. */
int lhip_debug_frac_call(const lhip_stream* s, size_t nsamples, int32_t* k, int32_t* frames);
int lhip_debug_frac_flush(const lhip_stream* s, int32_t* bytes, int32_t* clean, int cap);

const char* lhip_last_error(void);
const char* lhip_version(void);

#ifdef __cplusplus
}
#endif
#endif
