/* pocket_tts.h - C ABI of the MI355X-native Pocket TTS engine (variant b6369a24).
 *
 * This is the drop-in boundary for the reference's generation hot path. The
 * reference (ykevinc/pocket-tts, Rust/Candle) has no operator registry; the
 * seams it exposes are the model-level API of `TTSModel`
 * (crates/pocket-tts/src/tts_model.rs) and the kernel-level forwards of
 * `FlowLMModel` / `MimiModel`. Each entry point below names the reference
 * interface it replaces. Plain pointers and sizes only; the engine owns all
 * device memory, the caller owns host buffers. Every function returns 0 on
 * success or a PTTS_ERR_* code; `ptts_last_error()` gives a thread-local
 * message (the reference maps its anyhow::Error the same way at the FFI edge:
 * crates/pocket-tts-bindings/src/lib.rs:17).
 *
 * Threading: calls on one engine are externally serialized, as in the
 * reference (tts_model.py:315-316; server state.rs:69). One engine per GPU.
 *
 * Measurement and test hooks with no reference counterpart (per-kernel timing, the step plan,
 * the overlap probe, the GEMM-core test entry) are declared in pocket_tts_probe.h, not here:
 * this header is only the drop-in boundary a reference maintainer binds.
 */
#ifndef POCKET_TTS_H
#define POCKET_TTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTTS_OK 0
#define PTTS_ERR_INVALID 1 /* bad argument / shape */
#define PTTS_ERR_HIP 2     /* HIP runtime error (no GPU, OOM, launch failure) */
#define PTTS_ERR_STATE 3   /* call not valid in the current slot/engine state */
#define PTTS_ERR_IO 4      /* weights file missing or malformed */

/* ABI version of this header. Bumped whenever a struct below changes layout (3: cfg_yaml was
 * appended to ptts_engine_config; 4: back_frames; 5: back_bf16; 6: that field became back_mfma, with
 * the bf16x6 f32 mode). A caller checks ptts_abi_version() ==
 * PTTS_ABI_VERSION before passing any struct: a library built from another header reads a
 * different layout. */
#define PTTS_ABI_VERSION 6
int ptts_abi_version(void);
/* Build id of the loaded library: the first 16 hex digits of the sha256 over the sources it was
 * built from (pocket-tts_amd/Makefile, BUILD_ID), with "+probes" appended for a measurement build
 * (-DPTTS_PROBES). Lets a test harness refuse a stale prebuilt binary. */
const char* ptts_build_id(void);

#define PTTS_FRAME_SAMPLES 1920 /* 24 kHz / 12.5 Hz (config/b6369a24.yaml:24-27) */
#define PTTS_LATENT_DIM 32
#define PTTS_MODEL_DIM 1024
#define PTTS_SAMPLE_RATE 24000

typedef struct ptts_engine ptts_engine;
typedef struct ptts_voice ptts_voice;

typedef struct ptts_engine_config {
  int device;           /* HIP device ordinal (one engine per GPU) */
  int max_slots;        /* concurrent utterances (batch rows) */
  int max_ctx;          /* FlowLM KV capacity per slot, positions (voice + text + frames) */
  int lsd_decode_steps; /* TTSModel.lsd_decode_steps (tts_model.rs:22-49): the cap on every
                           utterance's own Euler step count, and the count of an utterance
                           admitted without one (ptts_slot_open_ex) */
  uint64_t synth_seed;  /* synthetic weights (tests/golden/synth.py rule) if weights_path == NULL */
  const char* weights_path; /* local safetensors with TTSModel state-dict names, or NULL */
  void* weight_blob;        /* optional caller-owned device buffer of ptts_weight_blob_bytes() */
  int defer_weights;        /* 1: leave the blob unfilled; caller fills it (e.g. RCCL broadcast)
                               and then calls ptts_engine_finalize() */
  int pipeline;             /* 0: each ptts_step returns the frame it computed.
                               1: overlapped stepping - the Mimi decode of frame k runs on a
                               second stream concurrently with the FlowLM step of frame k+1, so a
                               call returns the frame computed by the PREVIOUS call (one extra
                               call drains the last frame; the first call after admission
                               returns no frame for the admitted rows). */
  int weight_quant;         /* PTTS_QUANT_*: the reference's weight quantization (quantize.rs,
                               QuantizeConfig::default(): symmetric per-tensor int8 levels) applied
                               when the weights are packed (TTSModel::load_quantized*,
                               tts_model.rs:108-171). The FlowLM step GEMMs then stream int8 codes
                               (float(q) * scale rebuilt in-kernel = the simulated f32 weight).
                               A deferred blob must have been packed with the same mode. */
  int fp8_gemm;             /* 1: the large FlowLM step GEMMs (qkv, linear1, linear2, adaLN) run
                               as fp8 W8A8 on v_mfma_f32_32x32x16_fp8_fp8: OCP e4m3 weight codes
                               with one scale per output row, activations quantized in-kernel per
                               (row, K slice). Not a reference numeric (the reference has no fp8;
                               BASELINE configs[4]): gated on accuracy vs the f32 path. Requires
                               weight_quant = PTTS_QUANT_NONE. 0 = f32 (default). */
  const char* cfg_yaml;     /* the reference's model config (config/b6369a24.yaml; TTSModel::load's
                               config, config.rs:111-115), or NULL. The kernels implement the
                               b6369a24 dimensions; when given, every hot-path key of the file must
                               be present and equal them, or creation fails (PTTS_ERR_INVALID,
                               naming the key): another variant is a rebuild. Checked, not read
                               for shapes. ptts_config_check() is the same check alone. */
  int back_frames;          /* pipelined engines only: frames per Mimi-decode pass, 1 (default;
                               0 means 1), 2, 4 or 8. With n > 1, frames n j .. n j + n - 1 of every
                               row are decoded by ONE back pass (the streaming codec state advances
                               as for n passes; PCM identical within float rounding), a call
                               returns the frame computed 2 n - 1 calls earlier, and rows admitted
                               inside a pass start at the next pass boundary (an utterance's frames
                               group into passes from its first). ptts_frame_lag() reports both
                               delays. 2 is the throughput setting (bench.py's default; 4 measured
                               in DESIGN.md section 14), 1 the low-latency one. */
  int back_mfma;            /* PTTS_BACK_*: how the Mimi decoder transformer GEMMs and the SEANet
                               decoder convs (the back part, at >= 16 rows) use the matrix cores.
                               PTTS_BACK_F32 (0): v_mfma_f32_32x32x2_f32, an exact f32 FMA chain.
                               PTTS_BACK_F32X6 (2): f32 products on the bf16 matrix pipe: each f32
                               operand as the exact sum of three bf16 pieces, the six piece products
                               of order <= 2 summed in f32 (dropped terms < 2^-24 |a b|): f32
                               accuracy (the GEMM-core tests hold it to the f32 tile's error against
                               fp64), 6 bf16 MFMAs per 16 k instead of 8 f32 ones.
                               PTTS_BACK_BF16 (1): operands rounded to bf16, f32 accumulation: NOT a
                               reference numeric (Candle runs f32), gated on PCM accuracy.
                               The latents, EOS logits and stop frames never depend on it (the back
                               part does not feed the FlowLM). */
} ptts_engine_config;

#define PTTS_BACK_F32 0
#define PTTS_BACK_BF16 1
#define PTTS_BACK_F32X6 2

#define PTTS_QUANT_NONE 0
#define PTTS_QUANT_FLOW_LM 1 /* quantize_weights() over the flow_lm.* tensors */
#define PTTS_QUANT_ALL 2     /* ... over the whole state dict (Mimi included) */

/* Per-utterance generation parameters: TTSModel's public fields temp / eos_threshold /
 * noise_clamp (tts_model.rs:22-49) plus what generate_stream_segment derives from the text
 * (max_gen_len = (words+2)*13, frames_after_eos: tts_model.rs:968-969,1230-1237). */
typedef struct ptts_gen_params {
  float temp;            /* noise std = sqrt(temp); 0 = deterministic (flow_lm.rs:39-65) */
  float eos_threshold;   /* EOS when out_eos logit > threshold (flow_lm.rs:139-145) */
  float noise_clamp;     /* <= 0: None; else truncated normal |x| <= clamp */
  int frames_after_eos;  /* frames yielded after the EOS step (5 if <=4 words else 3) */
  int max_frames;        /* max_gen_len */
  uint64_t seed;         /* noise stream seed for this utterance */
} ptts_gen_params;

/* Size of the packed device weight blob (all tensors, engine layout). */
size_t ptts_weight_blob_bytes(void);
/* Pack the weights (synthetic from synth_seed when weights_path is NULL/empty, else a local
 * safetensors file with TTSModel state-dict names) into a host buffer of at least
 * ptts_weight_blob_bytes(), in the engine's device layout. Host only: no GPU needed. A
 * multi-GPU launcher packs once, broadcasts the blob (RCCL) into every rank's engine buffer
 * (cfg.weight_blob + defer_weights) and calls ptts_engine_finalize(). Replaces the per-process
 * VarBuilder load of TTSModel::load_with_params_device (tts_model.rs:86-106). */
int ptts_pack_weights(uint64_t synth_seed, const char* weights_path, float* host_out, size_t n_bytes);
/* The checkpoint tensors the packer reads, one line each: "name\tdim0,dim1,...\n" (TTSModel
 * state-dict keys: flow_lm.* and mimi.*, the VarBuilder prefixes of tts_model.rs:279-426, with the
 * checkpoint's own shapes). A weights file needs exactly these (extra tensors, e.g. the dropped
 * VQ codebooks, are ignored; F32, BF16 or F16). *needed = bytes incl. the terminating 0. Host only. */
int ptts_weight_manifest(char* buf, size_t cap, size_t* needed);
/* Same with the reference's weight quantization applied (weight_quant = PTTS_QUANT_*;
 * quantize.rs:126-150 quantize_weights with QuantizeConfig::default()). */
int ptts_pack_weights_ex(uint64_t synth_seed, const char* weights_path, int weight_quant, float* host_out,
                         size_t n_bytes);
/* The quantizer alone (QuantizedTensor::quantize, quantize.rs:66-90): out = simulated values,
 * *scale = the per-tensor scale. Host only. */
int ptts_quantize_tensor(const float* x, size_t n, int num_levels, float* out, float* scale);
/* 1 if quantize_weights() with QuantizeConfig::default() quantizes tensor `name` of `numel`
 * elements in scope `weight_quant` (should_skip_layer + min_size, quantize.rs:120-150). */
int ptts_quant_applies(const char* name, size_t numel, int weight_quant);
/* Number of FlowLM GEMM weight matrices the engine streams as int8 codes (0 when not quantized). */
int ptts_engine_int8_matrices(ptts_engine* e);
/* Number of FlowLM GEMM weight matrices running on the fp8 path (fp8_gemm = 1), else 0. */
int ptts_engine_fp8_matrices(ptts_engine* e);

/* TTSModel::load / load_with_params_device (tts_model.rs:59-106,182-236). */
int ptts_engine_create(const ptts_engine_config* cfg, ptts_engine** out);
/* The cfg_yaml check of ptts_engine_create without an engine (no GPU needed): 0 if the model
 * config at `cfg_yaml` states the dimensions this build implements (config.rs:1-124 keys). */
int ptts_config_check(const char* cfg_yaml);
/* Second half of create when cfg->defer_weights = 1 (derived tables, time embeddings). */
int ptts_engine_finalize(ptts_engine* e);
void ptts_engine_destroy(ptts_engine* e);
/* Copy a host blob from ptts_pack_weights[_ex] into a deferred engine's weight buffer (the
 * single-process alternative to a device-side fill); call ptts_engine_finalize() after it. */
int ptts_engine_load_blob(ptts_engine* e, const float* host_blob, size_t n_bytes);
/* Device pointer of the packed weight blob (for the caller's RCCL broadcast). */
void* ptts_engine_weight_blob(ptts_engine* e);

/* TTSModel::get_voice_state_from_prompt_tensor (tts_model.rs:490-501): prefill an
 * `audio_prompt` [n_frames x 1024] (row-major, host) into an immutable voice KV prefix. */
int ptts_voice_from_prompt(ptts_engine* e, const float* prompt, int n_frames, ptts_voice** out);
/* TTSModel::get_voice_state_from_tensor (tts_model.rs:504-560): 24 kHz mono PCM ->
 * Mimi encoder -> speaker projection -> FlowLM prefill. n_samples is zero-padded to a
 * multiple of 1920. */
int ptts_voice_from_pcm(ptts_engine* e, const float* pcm, int n_samples, ptts_voice** out);
/* The voice-cloning front end of TTSModel::get_voice_state / get_voice_state_from_bytes
 * (tts_model.rs:428-463) after the WAV decode, then get_voice_state_from_tensor (:504-577):
 * `n_samples` mono samples at `sample_rate` Hz are resampled to 24 kHz on the GPU by the
 * resample_poly rule of the Python reference's convert_audio (audio_utils.py:8-28: the rule the
 * reference's own ref.wav -> ref_mimi_input pair was made with), zero-padded to whole frames and
 * encoded. The Rust driver resamples with rubato's FastFixedIn instead (audio.rs:210-231), a
 * deliberate divergence: its parity with this path is unpinned.
 * chunk_frames = TTSModel.voice_prompt_chunk_frames: the encoder chunk length in frames; 0 = the
 * reference's adaptive rule (adaptive_voice_prompt_chunk_frames, tts_model.rs:562-577: whole
 * prompt up to 120 frames, then 120/180/240), < 0 = one pass (the Python reference,
 * tts_model.py:258-262). Each chunk re-applies the downsample conv's replicate padding, as the
 * Rust driver's step=0 per chunk does (tts_model.rs:536-541, conv.rs:116-123).
 * ptts_voice_from_pcm(e, pcm, n, out) == ptts_voice_from_audio(e, pcm, n, 24000, 0, out). */
int ptts_voice_from_audio(ptts_engine* e, const float* samples, int n_samples, int sample_rate, int chunk_frames,
                          ptts_voice** out);
/* The GPU resampler alone (audio.rs:197-255 `resample` for one channel): y receives
 * ptts_resample_len(n_samples, sr_from, sr_to) samples = ceil(n * up / down) with up/down the
 * rates divided by their gcd. */
int ptts_resample_len(int n_samples, int sr_from, int sr_to);
int ptts_resample(ptts_engine* e, const float* x, int n_samples, int sr_from, int sr_to, float* y);
/* Resampler choice of the _ex entry points below. PTTS_RESAMPLE_POLY is the rule above (the
 * default everywhere). PTTS_RESAMPLE_RUBATO_SEPTIC is the Rust driver's own resample()
 * (audio.rs:197-255): rubato 0.14.1 FastFixedIn, PolynomialDegree::Septic, ratio sr_to / sr_from,
 * one process() call over the whole input, output kept as rubato returns it (no delay
 * compensation, no trim). Its source is not in the reference: the restated algorithm (kernels.h
 * septic_schedule, oracle/ptts_oracle.c orc_resample_septic) is parity-unpinned. Equal rates
 * return the input unchanged for both, as audio.rs:198-200 does. */
#define PTTS_RESAMPLE_POLY 0
#define PTTS_RESAMPLE_RUBATO_SEPTIC 1
/* Output length of the chosen resampler (0 if the arguments are invalid); for the rubato rule the
 * count of its position walk, about (n - 5) * sr_to / sr_from. */
int ptts_resample_len_ex(int n_samples, int sr_from, int sr_to, int resampler);
int ptts_resample_ex(ptts_engine* e, const float* x, int n_samples, int sr_from, int sr_to, int resampler, float* y);
/* ptts_voice_from_audio with the resampler chosen; ptts_voice_from_audio(...) ==
 * ptts_voice_from_audio_ex(..., PTTS_RESAMPLE_POLY, out). */
int ptts_voice_from_audio_ex(ptts_engine* e, const float* samples, int n_samples, int sample_rate, int chunk_frames,
                             int resampler, ptts_voice** out);
/* Voice jobs: the clones above without draining the step pipeline. A job runs on a
 * stream of the engine's own (lowest priority) with a workspace of its own, in submission order;
 * admission is ordered behind it on the GPU by an event, with no host wait. */
#define PTTS_SAMPLES_F32 0
#define PTTS_SAMPLES_S16 1
/* Enqueue a clone of a mono clip on the engine's voice stream and return at once. *out is usable in
 * ptts_slot_open / ptts_slots_open[_ex] immediately (the admission is ordered behind the job on the
 * GPU). It is the clone ptts_voice_from_audio_ex makes, the same launches on another stream and
 * workspace: the same conditioning on the same samples (int16 samples: v / 32768), bit for bit.
 * Does not drain the step pipeline nor touch its buffers. `samples` is read before the call returns. All
 * arguments are checked before anything is enqueued: a rejected job leaves *out NULL. */
int ptts_voice_job_start(ptts_engine* e, const void* samples, int n_samples, int sample_format,
                         int sample_rate, int chunk_frames, int resampler, ptts_voice** out);
/* The same for a precomputed audio_prompt [n_frames x 1024] (get_voice_state_from_prompt_tensor). */
int ptts_voice_job_start_prompt(ptts_engine* e, const float* prompt, int n_frames, ptts_voice** out);
/* *ready = 1 once the voice's job has run (always 1 for a synchronously made voice and for a NULL
 * voice, which has no job); wait = 1 blocks until then. A NULL `ready` is PTTS_ERR_INVALID.
 * ptts_voice_len is valid as soon as the job is started; ptts_voice_conditioning and
 * ptts_voice_destroy wait for the job. */
int ptts_voice_ready(const ptts_voice* v, int wait, int* ready);
/* Pre-size the voice workspace for clips of up to max_frames frames (< max_ctx). Without it the
 * workspace is allocated at the first job and grows when a longer clip arrives (the voice stream,
 * never the step pipeline, is synchronized then). */
int ptts_voice_jobs_reserve(ptts_engine* e, int max_frames);
/* Conditioning rows the voice holds (frames). */
int ptts_voice_len(const ptts_voice* v);
/* The [n_frames x 1024] conditioning a PCM voice was built from (host copy); for tests. */
int ptts_voice_conditioning(const ptts_voice* v, float* out, int max_rows);
void ptts_voice_destroy(ptts_voice* v);

/* Admission of one utterance into batch row `slot` = the per-segment prologue of
 * generate_stream_segment (tts_model.rs:938-1004): copy the voice KV prefix, embed and
 * prefill `n_ids` text tokens (text.rs:289-303), reset the Mimi state, backbone = bos_emb. */
int ptts_slot_open(ptts_engine* e, int slot, const ptts_voice* v, const int32_t* ids, int n_ids,
                   const ptts_gen_params* p);
/* Batched admission of n utterances (distinct slots) in one call: voices[i], params[i] and
 * n_ids[i] tokens taken in order from the concatenated `ids`. Same per-row result as n
 * ptts_slot_open calls; the text prefills of all rows share one pass (the server admitting a
 * burst of requests, or a batch job starting). */
int ptts_slots_open(ptts_engine* e, int n, const int* slots, const ptts_voice* const* voices, const int32_t* ids,
                    const int* n_ids, const ptts_gen_params* params);
/* The same admissions with the utterance's own LSD Euler step count (the reference's
 * TTSModel.lsd_decode_steps, a field a caller may change between calls, and the server's per-request
 * lsd_steps): lsd_steps in [1, cfg.lsd_decode_steps], or 0 (for ptts_slots_open_ex also a NULL
 * array) for the engine's default, cfg.lsd_decode_steps; anything else is PTTS_ERR_INVALID and
 * admits nothing. Rows with different counts share one batched step, and each computes what an
 * engine created with lsd_decode_steps = its count would. ptts_slot_open, ptts_slots_open and
 * ptts_generate are these calls with the default. */
int ptts_slot_open_ex(ptts_engine* e, int slot, const ptts_voice* v, const int32_t* ids, int n_ids,
                      const ptts_gen_params* p, int lsd_steps);
int ptts_slots_open_ex(ptts_engine* e, int n, const int* slots, const ptts_voice* const* voices, const int32_t* ids,
                       const int* n_ids, const ptts_gen_params* params, const int* lsd_steps);
/* Wire-format output (no reference counterpart: the reference emits f32 at 24 kHz and its server
 * converts on the host, audio.rs:110-185). A row admitted with a wire format also gets, per frame,
 * the bytes a client reads: its PCM resampled to wire_rate by the resample_poly rule of
 * ptts_resample (streaming: the chunks of a row concatenate to the whole-signal resample of its
 * PCM, bit for bit; 24000 is the identity) and encoded as 16-bit little-endian integers by the wire
 * rule trunc(clamp(x, -1, 1) * 32767), or as the G.711 mu-law / A-law code of that 16-bit value.
 * The conversion runs on the GPU at the end of the back part; rows of every format and rows with
 * none share a batch, and the f32 PCM of ptts_fetch is unchanged for all of them. Chunk sizes in
 * samples (first / middle / last frame of an utterance): 8 kHz 630 / 640 / 650, 16 kHz 1270 /
 * 1280 / 1290, 44.1 kHz 3510 / 3528 / 3546, 48 kHz 3820 / 3840 / 3860, 24 kHz 1920; an
 * utterance of one frame emits 1920 * rate / 24000 at once. */
#define PTTS_WIRE_NONE 0
#define PTTS_WIRE_S16 1
#define PTTS_WIRE_ULAW 2
#define PTTS_WIRE_ALAW 3
#define PTTS_WIRE_CHUNK_MAX 8192 /* bytes: the largest chunk of one frame (3860 16-bit samples) fits */
/* on = 1: the engine's back passes end in the wire stage and one more device-to-host copy; 0: as
 * created (the same graphs and copies as an engine that never called this). Valid on an idle engine
 * before its first step, as ptts_preview_enable is; PTTS_ERR_INVALID later. */
int ptts_wire_enable(ptts_engine* e, int on);
/* Per-row admission options. size = sizeof(ptts_slot_opts) of the caller's header (0 is read as
 * 40, the struct that ended at keep_codec, as it was for callers built before pitch_cents: a caller
 * that sets pitch_cents states its size): the stride of the array, and fields past it read as 0, so the struct can grow
 * without an ABI bump. Zero fields are the defaults: lsd_steps as in ptts_slots_open_ex; wire_rate
 * 0 and wire_encoding 0: no wire format; one of them 0: 24000 / PTTS_WIRE_S16; speed_permille 0:
 * no speed (the field lies in what was the struct's tail padding: zero the struct before filling it).
 *
 * Latent prefix and codec continuity (no reference counterpart: the
 * reference starts every sentence chunk from fresh states and names teacher forcing as the better
 * way, tts_model.py:397-400). A row may be admitted behind n_prefix >= 0 latents p[0 .. n_prefix),
 * each [32], in FlowLM space (the values ptts_fetch returns in `latents`). It then starts in exactly
 * the state of a row that was admitted without a prefix and ran n_prefix steps in which each
 * sampled latent was replaced by p[j] before it became the next backbone input (what
 * ptts_slot_set_latent after each step does), with the outputs of those steps discarded. With F
 * voice rows and S tokens: FlowLM KV positions F+S .. F+S+n_prefix-1 hold the layers' K/V for the
 * inputs [bos, p[0], .., p[n_prefix-2]], the next position is F+S+n_prefix, and the backbone input
 * of the first step is p[n_prefix-1] (bos with no prefix). The generation counters count NEW frames
 * only: max_frames, the EOS tail (frames_after_eos) and the noise stream are indexed from the first
 * new frame; no EOS decision is taken inside the prefix, which runs no EOS head, no flow head and
 * no Mimi decode. The capacity rule is F + S + n_prefix + max_frames <= max_ctx.
 * keep_codec = 0: the Mimi state is fresh, as for every other admission. keep_codec = 1: the state
 * the slot's decoder ended on (attention ring and its position, the conv histories, the overlap-add
 * history) is NOT reset, so the first new frame is decoded as the continuation of the last frame
 * the slot decoded; frame flags, wire state and tempo state are reset as always (a request's wire
 * stream is its own). It needs no prefix (a seamless join without teacher forcing). It is valid
 * only on a slot whose previous utterance has had its last frame fetched, or on a never-used slot
 * (where it equals a fresh state): after ptts_slot_close or ptts_slots_cancel of an utterance on
 * the slot, or with frames still unfetched, it is PTTS_ERR_STATE and admits nothing. keep_codec
 * rows get no first-frame preview (a preview decodes from the fresh state). n_prefix < 0,
 * n_prefix > 0 with prefix_latents NULL, keep_codec outside {0, 1} or a failing capacity rule is
 * PTTS_ERR_INVALID and admits nothing. A caller with the older 24-byte struct gets neither. */
typedef struct ptts_slot_opts {
  size_t size;
  int lsd_steps;
  int wire_rate;     /* 8000, 16000, 24000, 44100 or 48000 */
  int wire_encoding; /* PTTS_WIRE_* */
  int speed_permille; /* speech speed, 500 .. 2000 (ptts_tempo_enable); 0 or 1000: none */
  const float* prefix_latents; /* host memory [n_prefix][32], read before the call returns */
  int n_prefix;
  int keep_codec;
  int pitch_cents; /* pitch shift, -1200 .. 1200 cents (ptts_pitch_enable); 0: none. Size 40 -> 48 */
  int reserved;    /* offset 44: what was the 48-byte struct's tail padding; ignored */
  int gain_cdb;    /* volume in hundredths of a dB, -2400 .. 2400 (ptts_level_enable); 0: none. Size 48 -> 56 */
  int limit;       /* 1: the row runs through the peak limiter even at gain 0; 0: only with a gain */
  int align;       /* 1: the row is in the align stage (ptts_align_enable); 0: not. Size 56 -> 64 */
  int reserved2;   /* ignored */
  int loud;        /* 1: the row is metered (ptts_loud_enable); 0: not. Size 64 -> 72 */
  int reserved3;   /* ignored */
} ptts_slot_opts;
/* ptts_slots_open_ex with one opts entry per row (NULL: defaults; the four admission calls above
 * are this call with defaults). A rate or encoding outside the lists, or a format asked of an
 * engine without ptts_wire_enable, is PTTS_ERR_INVALID and admits nothing. */
int ptts_slots_open_opts(ptts_engine* e, int n, const int* slots, const ptts_voice* const* voices, const int32_t* ids,
                         const int* n_ids, const ptts_gen_params* params, const ptts_slot_opts* opts);
/* The wire seam alone, like ptts_resample: bytes of n_samples at 24 kHz in the format (0 if the
 * arguments are invalid; host only), and the whole-signal conversion on the GPU (the kernel
 * ptts_resample runs, then the encoder of the streaming stage); out receives ptts_wire_len bytes. */
long ptts_wire_len(long n_samples, int sample_rate, int encoding);
int ptts_wire_encode(ptts_engine* e, const float* pcm, int n_samples, int sample_rate, int encoding, uint8_t* out);
/* Speech speed (no reference counterpart; the model has no duration control). A row admitted with
 * ptts_slot_opts.speed_permille = sp has its f32 PCM time-scaled at 24 kHz ahead of the wire
 * conversion, by a streaming WSOLA whose rule DESIGN.md section 19 states: pitch is kept, an
 * utterance of N samples becomes ceil(N * 1000 / sp), and the chunks of a row concatenate to the
 * whole-signal rule (ptts_tempo) over its PCM, bit for bit. Only the wire bytes change: the PCM of
 * ptts_fetch, the latents, the EOS logits and the stop frames do not depend on speed. A speed with
 * no wire format implies 24000 / PTTS_WIRE_S16. A speed outside [500, 2000], or one asked of an
 * engine without ptts_tempo_enable, is PTTS_ERR_INVALID and admits nothing.
 * ptts_tempo_enable: valid on a wire-enabled idle engine before its first step (PTTS_ERR_INVALID
 * otherwise); on = 0, or never called: the passes, graphs and copies of a wire-enabled engine. On a
 * tempo-enabled engine chunks can be longer (a last frame at speed 500 and 48 kHz holds 11,058
 * 16-bit samples at most), and ptts_fetch_wire requires row_stride >= PTTS_WIRE_CHUNK_MAX_TEMPO. */
#define PTTS_WIRE_CHUNK_MAX_TEMPO 22528
int ptts_tempo_enable(ptts_engine* e, int on);
/* The tempo seam alone: samples of n at speed sp (0 if the arguments are invalid; host only), and
 * the whole-signal rule on the GPU (the hop functions of the streaming stage); out receives
 * ptts_tempo_len samples. */
long ptts_tempo_len(long n, int speed_permille);
int ptts_tempo(ptts_engine* e, const float* pcm, int n, int speed_permille, float* out);
/* Pitch (no reference counterpart; the model has no pitch input). A row admitted with
 * ptts_slot_opts.pitch_cents = c (-1200 .. 1200; 0: none, today's bytes) has its wire bytes shifted
 * in pitch by 2^(c / 1200) at the duration its speed asks for, by the rule of DESIGN.md section 23:
 * the WSOLA stage runs at wsola_permille = round(speed * 2^20 / step) and a streaming windowed-sinc
 * resampler then reads step_q20 / 2^20 input samples per output sample, step_q20 =
 * round(2^(c / 1200) * 2^20). It is a resampling shift: formants move with the fundamental. The
 * chunks of a row concatenate to the whole-signal rule (ptts_tempo, then ptts_pitch_resample) over
 * its PCM, bit for bit; only the wire bytes change (the PCM of ptts_fetch, the latents, the EOS
 * logits and the stop frames do not depend on pitch). A pitch with no wire format implies 24000 /
 * PTTS_WIRE_S16. A pitch outside the range, one whose wsola_permille leaves [500, 2000], or one asked
 * of an engine without ptts_pitch_enable, is PTTS_ERR_INVALID and admits nothing. A caller with a
 * struct shorter than 48 bytes gets none.
 * ptts_pitch_enable: valid on a tempo-enabled idle engine before its first step (PTTS_ERR_INVALID
 * otherwise); on = 0, or never called: the passes, graphs and copies the engine has without it. The
 * chunk slots stay PTTS_WIRE_CHUNK_MAX_TEMPO (a last frame at 48 kHz holds 11,196 16-bit samples at
 * most). */
int ptts_pitch_enable(ptts_engine* e, int on);
/* The pitch seam alone. ptts_pitch_plan (host only): the plan of (cents, speed_permille; 0: 1000),
 * PTTS_ERR_INVALID for an invalid request; either pointer may be NULL. ptts_pitch_len (host only):
 * floor(n 2^20 / step_q20) (0 if the arguments are invalid). ptts_pitch_table (host only): the
 * prototype table T and its differences D, n = 16385 entries each. ptts_pitch_resample: the
 * whole-signal rule on the GPU (the tap loop of the streaming stage), step_q20 in [2^19, 2^21]; y
 * receives ptts_pitch_len samples. */
int ptts_pitch_plan(int cents, int speed_permille, int* wsola_permille, uint32_t* step_q20);
long ptts_pitch_len(long n, uint32_t step_q20);
int ptts_pitch_table(float* t, float* d, int n);
int ptts_pitch_resample(ptts_engine* e, const float* x, int n, uint32_t step_q20, float* y);
/* Volume and peak limiting (no reference counterpart). A row admitted with ptts_slot_opts.gain_cdb
 * != 0 or .limit == 1 is in the level stage: between the pitch stage and the
 * wire stage its samples x (f32 at 24 kHz, after speed and pitch) become u = v x with v =
 * (float)pow(10, gain_cdb / 2000), and a look-ahead peak limiter of 126 samples (5.25 ms) keeps the
 * result inside the engine's ceiling C = (float)pow(10, ceiling_cdb / 2000): r[n] = |u[n]| > C ? C /
 * |u[n]| : 1, m[i] = min(r[i .. i + 126]), g[n] = (float)(sum_{k = 0..126} (64 - |k - 63|) m[n - k] /
 * 4096) summed in f64, y[n] = clamp(g[n] u[n], -C, C). Where no |u| within 126 samples exceeds C the
 * output is v x exactly. The output has the input's length; a streaming row emits 126 samples late and
 * catches up in its last frame, and its chunks concatenate to the whole-signal rule (ptts_level) over
 * the stage's input, bit for bit. Only the wire bytes change. A gain or limit with no wire format
 * implies 24000 / PTTS_WIRE_S16. A gain outside [-2400, 2400], a limit outside {0, 1}, or either asked
 * of an engine without ptts_level_enable, is PTTS_ERR_INVALID and admits nothing. A caller with a
 * struct shorter than 56 bytes gets neither.
 * ptts_level_enable: valid on a wire-enabled idle engine before its first step (PTTS_ERR_INVALID
 * otherwise, or for ceiling_cdb outside [-4000, 0]); independent of the tempo and pitch stages; on =
 * 0, or never called: the passes, graphs and copies the engine has without it. On a level-enabled
 * engine a last chunk holds up to 252 more samples at 48 kHz (4,112 for a plain row, 11,448 behind
 * the pitch stage), every row's chunk slot is PTTS_WIRE_CHUNK_MAX_LEVEL bytes and ptts_fetch_wire
 * requires row_stride >= that. */
#define PTTS_WIRE_CHUNK_MAX_LEVEL 23552
int ptts_level_enable(ptts_engine* e, int on, int ceiling_cdb);
/* The level seam alone. ptts_level_plan (host only): the two f32 factors of (gain_cdb, ceiling_cdb),
 * PTTS_ERR_INVALID outside the ranges; either pointer may be NULL. ptts_level: the whole-signal rule
 * on the GPU (the window function of the streaming stage), n >= 1; y receives n samples. */
int ptts_level_plan(int gain_cdb, int ceiling_cdb, float* gain, float* ceiling);
int ptts_level(ptts_engine* e, const float* x, int n, int gain_cdb, int ceiling_cdb, float* y);
/* Loudness (no reference counterpart; ITU-R BS.1770 / EBU R128, restated in DESIGN.md section 27). A
 * row admitted with ptts_slot_opts.loud = 1 is metered: the f32 signal at 24 kHz that the wire stage
 * reads for it (behind speed, pitch and level) runs through the K-weighting at 24 kHz in f64, and
 * for every complete sub-block of 2,400 samples (100 ms) of the row the pass reports the energy sum
 * of y^2, at most PTTS_LOUD_BLOCKS_MAX per frame. Samples behind the row's last complete sub-block
 * are never measured. The energies of a row, concatenated over its frames, are the whole-signal
 * rule (ptts_loud_blocks) over that signal, bit for bit as f64. The meter only reads: no other
 * output depends on it. A metered row with no wire format gets 24000 / PTTS_WIRE_S16. loud outside
 * {0, 1}, or loud = 1 on an engine without ptts_loud_enable, is PTTS_ERR_INVALID and admits nothing.
 * A caller with a struct shorter than 72 bytes gets no meter.
 * ptts_loud_enable: valid on a wire-enabled idle engine before its first step (PTTS_ERR_INVALID
 * otherwise); independent of the tempo, pitch, level and FLAC stages; on = 0, or never called: the
 * passes, graphs and copies the engine has without it.
 * ptts_fetch_loud: the companion of ptts_fetch / ptts_fetch_prev like ptts_fetch_wire (the same
 * call, the same event, no bookkeeping of its own): per row the sub-blocks its frame of that call
 * completed and their energies (unused entries 0). PTTS_ERR_INVALID on an engine without the stage. */
#define PTTS_LOUD_SUB 2400
#define PTTS_LOUD_BLOCKS_MAX 3
int ptts_loud_enable(ptts_engine* e, int on);
int ptts_fetch_loud(ptts_engine* e, int calls_back, int n_rows, double* energy /* [n_rows][3] */, int* n_blocks /* [n_rows] */);
/* The loudness seam alone. ptts_loud_coeffs (host only): c = shelf b0 b1 b2 a1 a2, high-pass b0 b1
 * b2 a1 a2 at 24 kHz; p_q = [biquad][p, q][32], the correction tables; either pointer may be NULL.
 * ptts_loud_len: sub-blocks of n samples, n / 2400 (0 for n < 0). ptts_loud_blocks: the whole-signal
 * rule on the GPU (the block function of the streaming stage); energy receives ptts_loud_len(n)
 * doubles. ptts_loud_integrated (host only): the gated loudness in LUFS of n sub-block energies (400
 * ms blocks of four, 75 % overlap, the absolute gate at -70 and the relative gate 10 LU below the
 * mean); *measurable = 0 and *lufs untouched with fewer than four sub-blocks or when the absolute
 * gate keeps nothing. */
int ptts_loud_coeffs(double* c /* [10] */, double* p_q /* [2][2][32] */);
long ptts_loud_len(long n);
int ptts_loud_blocks(ptts_engine* e, const float* x, int n, double* energy);
int ptts_loud_integrated(const double* energy, int n, double* lufs, int* measurable);
/* FLAC (no reference counterpart; RFC 9639, restated in DESIGN.md section 21). A row admitted with
 * wire_encoding = PTTS_WIRE_FLAC gets, per frame, the FLAC frames of the 16-bit samples its
 * PTTS_WIRE_S16 chunk at the same rate (and speed) would hold: mono, 16 bit, blocks of at most 4,608
 * samples (one frame per chunk; up to three on a tempo-enabled engine), fixed predictors of order
 * 0..4 with partitioned Rice codes chosen by the deterministic rule of section 21, CONSTANT or
 * VERBATIM subframes where they are cheaper. The frames carry the index of their first sample within
 * the row's utterance (variable-blocksize strategy), counted from 0 at the admission, so a row's
 * chunks behind a STREAMINFO header (42 bytes, built by the caller: min / max blocksize 16 / 4608,
 * the row's rate, 1 channel, 16 bits) are a complete stream that decodes to exactly those samples.
 * The encoder runs on the GPU behind the wire stage and writes over the chunk slot; a chunk of n
 * samples is at most ptts_flac_bound(n) = 2 n + 17 ceil(n / 4608) bytes, which fits the chunk slots
 * of ptts_fetch_wire. Only the row's wire bytes change: its f32 PCM, latents and flags, and every
 * other row, are what they are without it. PTTS_WIRE_FLAC asked of an engine without
 * ptts_flac_enable is PTTS_ERR_INVALID and admits nothing; ptts_wire_len returns 0 for it and
 * ptts_wire_encode rejects it (the size is not a function of n).
 * ptts_flac_enable: valid on a wire-enabled idle engine before its first step (PTTS_ERR_INVALID
 * otherwise); on = 0, or never called: the passes, graphs and copies the engine has without it. */
#define PTTS_WIRE_FLAC 4
int ptts_flac_enable(ptts_engine* e, int on);
/* The FLAC seam alone: the bound above (0 for n < 1; host only), and the stage's chunk encoder on
 * n <= 11,477 arbitrary 16-bit samples at sample_rate (one of the wire rates), the first of which
 * has index first_sample (0 <= first_sample, first_sample + n <= 2^36) in its stream; out holds
 * ptts_flac_bound(n) bytes, *n_bytes receives the frames' byte total. */
long ptts_flac_bound(long n);
int ptts_flac_encode(ptts_engine* e, const int16_t* samples, int n, int sample_rate, long long first_sample,
                     uint8_t* out, int* n_bytes);
/* The frame index. A chunk is at most three frames and carries no length
 * field, so the FLAC stage writes, beside each chunk, every frame's byte length and block size.
 * ptts_fetch_flac_index is the companion of ptts_fetch_wire (the same calls_back, rows and event, no
 * bookkeeping of its own): index[b][i] = {byte length, block size} of frame i of row b's chunk for
 * i < n_frames[b], zeros behind; n_frames[b] is 0 for a row that is not FLAC and for a slot with no
 * chunk, and the lengths of a chunk's frames sum to the n_bytes[b] of ptts_fetch_wire.
 * PTTS_ERR_INVALID on an engine without ptts_flac_enable. ptts_flac_encode_ex is ptts_flac_encode
 * with the index of its frames (index [3][2] and n_frames: both, or both NULL). */
int ptts_fetch_flac_index(ptts_engine* e, int calls_back, int n_rows, int* index /* [n_rows][3][2] */,
                          int* n_frames /* [n_rows] */);
int ptts_flac_encode_ex(ptts_engine* e, const int16_t* samples, int n, int sample_rate, long long first_sample,
                        uint8_t* out, int* n_bytes, int* index, int* n_frames);
/* Joining segments (host only: no engine, no GPU). A row numbers its frames from sample 0 of its own
 * utterance; a response of several rows and pauses is one stream when every frame's number is moved
 * to its place. ptts_flac_rebase writes the n_frames frames at `in` (n_bytes in all; index
 * [n_frames][2] as above) to `out` with the coded sample number of each raised by delta >= 0, in its
 * shortest form, and the CRC-8 and CRC-16 renewed; the body bits are untouched (moved by whole bytes
 * where the number's width changes), so a frame grows by at most 6 bytes: out_cap >= n_bytes +
 * 6 n_frames. `in` and `out` must not overlap. Everything is checked before the first byte is
 * written; PTTS_ERR_INVALID (and `out` untouched) for a frame that does not start with FF F9 or is
 * not a header of section 21.1, a CRC-8 or CRC-16 that does not verify, index lengths that do not sum
 * to n_bytes, a block size that differs from the index, delta < 0, a number + delta + block size
 * above 2^36, or a short out_cap.
 * ptts_flac_silence writes n >= 0 zero samples at sample_rate (one of the wire rates) as CONSTANT
 * frames in blocks of 4,608, the last one shorter, numbered from first_sample (first_sample + n <=
 * 2^36): the frames of section 21's rule on zeros. out_cap >= ptts_flac_silence_bound(n) =
 * 19 ceil(n / 4608) (0 for n < 1). */
int ptts_flac_rebase(const uint8_t* in, int n_bytes, const int* index, int n_frames, long long delta, uint8_t* out,
                     int out_cap, int* out_bytes);
long ptts_flac_silence_bound(long long n);
int ptts_flac_silence(long long n, int sample_rate, long long first_sample, uint8_t* out, long out_cap, long* out_bytes);

/* *cap: cfg.lsd_decode_steps. *last_run: the Euler steps the most recent step call ran (0 before
 * the first): the largest count among that call's rows still open (admitted, not closed, last
 * frame not yet fetched), so a call whose open rows all use one step pays for one. Either pointer
 * may be NULL. */
int ptts_lsd_steps(const ptts_engine* e, int* cap, int* last_run);
int ptts_slot_close(ptts_engine* e, int slot);
/* Stop the utterances of n distinct slots without draining the pipeline (ptts_slot_close waits for
 * every queued call; this call waits for nothing on the GPU). It is stream-ordered like an
 * admission: the slots go idle behind the step calls already issued, and the other rows are not
 * touched. From its return, ptts_fetch / ptts_fetch_prev / ptts_fetch_wire / ptts_preview_fetch
 * report no frame of a cancelled utterance (frame_valid 0, n_bytes 0, never `last`): frames of it
 * still in flight are dropped by their call index, frames of the slot's previous or next utterance
 * are not. A cancelled slot may be admitted again at once. Cancelling an idle, finished or
 * never-admitted slot is a no-op. A slot out of range or named twice is PTTS_ERR_INVALID and
 * cancels nothing. */
int ptts_slots_cancel(ptts_engine* e, int n, const int* slots);

/* THE batched hot path: one iteration of the loop body of generate_stream_segment
 * (tts_model.rs:1006-1070) for rows [0, n_rows): FlowLM step -> EOS -> flow sampling ->
 * denorm/quantize -> Mimi decode -> 1920 PCM samples per active row.
 * Host outputs (each may be NULL):
 *   pcm [n_rows x 1920], frame_valid [n_rows] (row was active this step),
 *   last [n_rows] (this was the row's final frame: EOS tail reached or max_frames),
 *   eos_logits [n_rows], latents [n_rows x 32] (the sampled latent of this step). */
int ptts_step(ptts_engine* e, int n_rows, float* pcm, uint8_t* frame_valid, uint8_t* last,
              float* eos_logits, float* latents);
/* Same step, enqueued only (outputs stay in HBM); use ptts_sync() + ptts_fetch(). */
int ptts_step_async(ptts_engine* e, int n_rows);
/* Pipelined engines: a call that starts no frame. The frames already computed advance through
 * the back part and are returned as by ptts_step_async (fetch after it as usual), but no row
 * computes a new frame: every row pauses for this call, as rows past n_rows do. A caller whose
 * rows have all finished drains the pipeline with it (ptts_frame_lag() calls) without running
 * front parts whose frames would be discarded. Not valid right after an admission
 * (PTTS_ERR_INVALID: the admitted rows' first frame must fall on a step call). No reference
 * counterpart (the reference does not pipeline). */
int ptts_flush_async(ptts_engine* e, int n_rows);
int ptts_sync(ptts_engine* e);
int ptts_fetch(ptts_engine* e, int n_rows, float* pcm, uint8_t* frame_valid, uint8_t* last,
               float* eos_logits, float* latents);
/* Calls by which a frame trails the call that computed its FlowLM step: 0 (sequential), 1
 * (pipelined), 2 n - 1 (pipelined, back_frames = n > 1). *admit_delay (may be NULL): the calls by
 * which the rows of the latest admission start late (back_frames = n > 1, admitted at a call k with
 * k % n != 0: n - k % n), else 0. A row admitted before call k returns its first frame from call
 * k + lag + admit_delay. */
int ptts_frame_lag(const ptts_engine* e, int* admit_delay);
/* ptts_fetch of an earlier call: calls_back = 0 is the latest call (= ptts_fetch), 1 the call
 * before it. Lets a driver keep one call in flight (issue call k+1, then fetch call k) so that the
 * GPU always has the next step queued while the host hands out frames. calls_back <= 1. */
int ptts_fetch_prev(ptts_engine* e, int calls_back, int n_rows, float* pcm, uint8_t* frame_valid, uint8_t* last,
                    float* eos_logits, float* latents);
/* The wire chunks of the same call's frame (the companion of ptts_fetch / ptts_fetch_prev: the same
 * event, no bookkeeping of its own, so call it beside them in either order): row b's n_bytes[b]
 * bytes at out + b * row_stride (row_stride >= PTTS_WIRE_CHUNK_MAX, or PTTS_WIRE_CHUNK_MAX_TEMPO on a
 * tempo-enabled engine); n_bytes[b] = 0 for a row with no
 * wire format or no frame. out may be NULL (sizes only). Wire-enabled engines only. */
int ptts_fetch_wire(ptts_engine* e, int calls_back, int n_rows, uint8_t* out, size_t row_stride, int* n_bytes);
/* Word alignment (no reference counterpart). On an align-enabled engine a row
 * admitted with ptts_slot_opts.align = 1 and S = n_ids <= PTTS_ALIGN_TOKENS tokens gets, with every
 * frame, the attention its FlowLM query of that step paid to its S text tokens in layer `layer`:
 * per head h of head_mask (bit h = head h of 16), the softmax over the text keys alone (KV
 * positions F .. F+S-1, F the voice rows) of q_h . k_j / 8, averaged over the selected heads. The
 * S values are >= 0 and sum to 1. One more launch in the FlowLM step computes them; every other
 * output of the engine is bit for bit what it is without the stage. The host rule that turns the
 * frames' rows into word times is pocket_tts_amd/align.py.
 * ptts_align_enable: valid on an idle engine before its first step, as ptts_wire_enable
 * (PTTS_ERR_INVALID later); a layer outside 0..5 or a mask without a bit among the 16 heads is
 * PTTS_ERR_INVALID. on = 0, or never called: the graphs and copies the engine has without it.
 * align = 1 on an engine without the stage, or with n_ids > PTTS_ALIGN_TOKENS, is PTTS_ERR_INVALID
 * and admits nothing.
 * ptts_fetch_align: the companion of ptts_fetch / ptts_fetch_prev like ptts_fetch_wire (the same
 * call's frame, the same event): row b's n_tokens[b] floats at out + b * row_stride (row_stride >=
 * PTTS_ALIGN_TOKENS, in floats); n_tokens[b] = 0 for a row with no valid frame or not in the
 * stage. The count is the one the device wrote beside the row. out may be NULL (counts only). */
#define PTTS_ALIGN_TOKENS 128
int ptts_align_enable(ptts_engine* e, int on, int layer, unsigned head_mask);
int ptts_fetch_align(ptts_engine* e, int calls_back, int n_rows, float* out, size_t row_stride, int* n_tokens);
/* *ready = 1 if ptts_fetch_prev(e, calls_back, ..) would return without waiting (the call's frame
 * is complete), else 0; never blocks. A driver that also serves previews polls this and
 * ptts_preview_fetch instead of blocking in the fetch. */
int ptts_fetch_ready(ptts_engine* e, int calls_back, int* ready);
/* *done = 1 once the FlowLM step (front part) of the call calls_back (0..3) calls before the latest
 * has run on the GPU; wait = 1 blocks until it has. Pipelined engines let the host run calls ahead
 * of the GPU; a driver that admits new rows waits here (calls_back = 1) before its next call, so an
 * admission queues behind one FlowLM step at most (first-chunk latency), while the GPU still has
 * the next step queued. Calls are tracked from an engine's first ptts_front_done on (each later
 * call records an event after its front part; a driver that never asks pays no marker per call):
 * a call issued before that is answered from the front stream as a whole (done once everything
 * queued on it has run), which can only be later, never earlier, than its own front part. */
int ptts_front_done(ptts_engine* e, int calls_back, int wait, int* done);
/* First-frame previews (pipelined engines; no reference counterpart: the reference decodes each
 * frame right after its FlowLM step, tts_model.rs:1040-1047, and does not pipeline). With
 * max_rows > 0 (at most 8), the first frame of up to max_rows rows that start in one call is also
 * decoded right after that call's FlowLM step, alone, from the fresh Mimi state every utterance
 * starts from, so the first chunk of a new stream does not wait ptts_frame_lag() calls. The rows'
 * regular first frame still arrives through ptts_fetch (within float rounding of the preview); a
 * caller delivers whichever comes first. 0 disables. PTTS_ERR_INVALID on a sequential engine. */
int ptts_preview_enable(ptts_engine* e, int max_rows);
/* Completed previews, oldest first: *n_out frames, slot slots[i] and pcm [i][1920] (at most
 * max_n; a preview's rows are returned together). wait = 0: only those already complete (never
 * blocks); 1: blocks until the launched previews complete (as many as fit in max_n). A slot
 * re-admitted or closed before its preview is fetched drops that preview. */
int ptts_preview_fetch(ptts_engine* e, int wait, int max_n, int* slots, float* pcm, int* n_out);
/* Test hook (teacher forcing): overwrite the backbone input latent of `slot`. */
int ptts_slot_set_latent(ptts_engine* e, int slot, const float* latent32);
/* MimiModel::decode_from_latent (mimi.rs:143-157) after the denorm + DummyQuantizer of
 * tts_model.rs:1033-1038 (the kernel-level seam of SURVEY §8(b)): n_frames FlowLM latents
 * [n][32] decoded in sequence on `slot`'s streaming state, which is reset first; every pending
 * frame of the engine is dropped (call on an idle engine). Outputs (each optional, NULL = skip):
 * pcm [n][1920]; quantized [n][512]; after_upsample and after_transformer [n][16][512]
 * (time-major; the reference's tensors are [1][512][16]). */
int ptts_decode_latents(ptts_engine* e, int slot, const float* latents, int n_frames, float* pcm, float* quantized,
                        float* after_upsample, float* after_transformer);

/* TTSModel::generate for one segment (tts_model.rs:687-703) on row `slot`: loops ptts_step
 * until the row's last frame. pcm_out receives up to max_samples samples. */
int ptts_generate(ptts_engine* e, int slot, const ptts_voice* v, const int32_t* ids, int n_ids,
                  const ptts_gen_params* p, float* pcm_out, int max_samples, int* n_samples);

const char* ptts_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
