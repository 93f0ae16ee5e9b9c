/*
 * dsm.h — C ABI of libdsm_mi355x.so: the MI355X-native replacement for the per-80 ms-frame
 * batched step of moshi-server's BatchedAsr worker (reference: /root/reference,
 * server/rust/moshi/moshi-server/src/batched_asr.rs calling into moshi-core).
 *
 * The reference boundary is a Rust API (no FFI exists upstream).  Each entry point below
 * names the Rust call it replaces; INTEGRATION.md shows the `extern "C"` shim a maintainer
 * adds on the Rust side.  Plain pointers and sizes only — no torch / candle types.
 *
 * Conventions
 *   - return 0 on success, <0 on error (DSM_ERR_*); dsm_last_error() gives the message.
 *     The reference bubbles candle::Error up and kills the loop thread
 *     (srv/utils.rs:376-384); here the caller decides.
 *   - the caller owns every host buffer; the engine owns all device memory.
 *   - B = batch_size = number of stream slots; one frame = 1920 f32 samples @ 24 kHz = 80 ms
 *     (srv/batched_asr.rs:26).
 *   - mask[b] != 0  <=>  slot b is active this step (core/streaming.rs:20-68 StreamMask).
 *   - threading: like the reference, dsm_mimi_encode_step may run on an "encoder" thread
 *     while dsm_asr_step_tokens / dsm_asr_reset_slot run on a "model" thread
 *     (srv/batched_asr.rs:314-522); the two sides use separate HIP streams and state.
 *
 * Environment
 *   The library reads exactly ten variables, once per engine at create (dsm_read_env, csrc/dsm_engine.hip).  Every value
 *   gives the same bits; they choose among launch sequences.  STT = dsm_asr_create*, TTS = dsm_tts_create.
 *   deployment switches
 *     DSM_GRAPHS          1     0: every launch sequence is enqueued kernel by kernel instead of replayed as a hipGraph
 *     DSM_LM_GROUPS       2 from 32 slots, else 1   STT: stream groups of the LM step (1..4)
 *     DSM_TTS_GROUPS      2 from 96 slots, else 1   TTS: stream groups of the step (1..4)
 *     DSM_FUSE_QKV        1     0: a split-K QKV (or cross-attention query) GEMM keeps its own reduce launch instead of
 *                               leaving the slabs to the attention kernel's prologue
 *     DSM_STREAM_PRIO     0     1: STT: LM streams at high, encoder stream at low priority (TTS: ignored, its streams
 *                               have no priorities)
 *   test levers (they push the large-batch kernels through small shapes; not for deployments)
 *     DSM_CHUNK_LOOP_MIN  384; STT in dot_mode 1: 192   whole-K-in-the-workgroup GEMMs from this many 64 x 64 tiles on
 *     DSM_LOOP_DEPTH      4     2: those GEMMs' rolling load window holds two blocks instead of four
 *     DSM_SMALLK_MIN      1024  one-chunk GEMMs (K <= 256) run on the loop kernel from this many 64-row tiles on
 *     DSM_SMALLK_MT       4     16-row tiles per workgroup of those launches (1, 2 or 4)
 *     DSM_FUSE_FRONT      1     0: the SEANet front end as three GEMM launches instead of the one fused kernel (same bits;
 *                               what tests compare the fused kernel against)
 */
#ifndef DSM_H
#define DSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_FRAME_SIZE 1920 /* srv/batched_asr.rs:26 FRAME_SIZE */
#define DSM_MAX_RATIOS 8
#define DSM_MAX_EXTRA_HEADS 8

enum {
  DSM_OK = 0,
  DSM_ERR_INVALID = -1,  /* bad argument / config (candle::bail! paths) */
  DSM_ERR_IO = -2,       /* weight file missing / malformed / tensor key or shape mismatch */
  DSM_ERR_DEVICE = -3,   /* HIP error */
  DSM_ERR_STATE = -4     /* call sequence the reference would reject */
};

/* transformer::Config — core/transformer.rs:21-53 (fields the batched path reads). */
typedef struct dsm_transformer_config {
  int d_model;
  int num_heads;
  int num_layers;
  int dim_feedforward;
  int context;          /* ring KV-cache length (core/kv_cache.rs:88-93) */
  int max_period;       /* RoPE theta (core/batched_transformer.rs:385-389) */
  int gating;           /* 0 = None (linear1/gelu_erf/linear2), 1 = silu gating (core/batched_transformer.rs:142-179) */
  int norm;             /* 0 = LayerNorm eps 1e-5, 1 = RmsNorm eps 1e-8 (core/batched_transformer.rs:236-252) */
  int positional_embedding; /* 0 = None, 1 = Rope */
  int layer_scale;      /* 0 = absent, 1 = layer_scale_{1,2}.scale present (core/batched_transformer.rs:291-304) */
  int conv_layout;      /* 1 = caller layout is [B,C,T] (Mimi), 0 = [B,T,C] (core/batched_transformer.rs:584-602) */
} dsm_transformer_config;

/* seanet::Config + mimi::Config — core/seanet.rs:12-31, core/mimi.rs:17-93 (v0_1 values in comments). */
typedef struct dsm_mimi_config {
  int channels;              /* 1 */
  int dimension;             /* 512 */
  int n_filters;             /* 64 */
  int n_residual_layers;     /* 1 */
  int n_ratios;              /* 4 */
  int ratios[DSM_MAX_RATIOS];/* {8,6,5,4} — the ENCODER applies them reversed (core/seanet.rs:194) */
  int kernel_size;           /* 7 */
  int residual_kernel_size;  /* 3 */
  int last_kernel_size;      /* 3 */
  int dilation_base;         /* 2 */
  int compress;              /* 2 */
  dsm_transformer_config transformer; /* d 512, 8 heads, 8 layers, ffn 2048, ctx 250, theta 10000, LayerNorm, layer_scale, conv_layout */
  int quantizer_n_q;         /* 32 for STT (srv/batched_asr.rs:754-757), 16 default */
  int quantizer_bins;        /* 2048 */
  int quantizer_dim;         /* 256 */
  int downsample_stride;     /* encoder_frame_rate / frame_rate = 25 / 12.5 = 2 (core/mimi.rs:141-144) */
} dsm_mimi_config;

/* ModuleConfig::BatchedAsr + lm::Config — srv/main.rs:110-128,179-184, core/lm.rs:36-46. */
typedef struct dsm_asr_config {
  dsm_transformer_config lm;
  int text_in_vocab_size;
  int text_out_vocab_size;
  int audio_vocab_size;
  int audio_codebooks;
  int extra_heads_num;   /* [modules.asr.model.extra_heads] num_heads (0 if absent) */
  int extra_heads_dim;
  int asr_delay_in_tokens;
  float temperature;     /* <= 0: argmax; > 0 (r04): candle_nn::sampling::gumbel_softmax (core/asr.rs:211-215) with a seeded ChaCha12
                            stream per slot (dsm_asr_set_seed) — the reference draws from an unseeded device generator: unpinnable */
  dsm_mimi_config mimi;
  /* engine numerics: 1 = K/V ring cache stored as bf16 (GPU target, BASELINE.md roofline),
   * 0 = f32 cache (the Candle CPU path's dtype, srv/utils.rs:386-395). */
  int kv_bf16;
  /* how the bf16-weight linear layers (the LM's GEMMs) form their dot products — both orders are restated bit for bit by the
   * oracle (oracle/dsm_oracle.c orc_dot), neither is Candle's (whose gemm order is implementation-defined):
   *   0  v_mfma_f32_16x16x4_f32: one f32 fmaf chain per 256-wide K-chunk (csrc/dsm_numerics.h)
   *   1  "bx3" (r03): the f32 activation split exactly into three bf16 pieces, v_mfma_f32_16x16x32_bf16 on (weight, piece)
   *      per 32-wide block in the order lo, mid, hi; the instruction's internal adder as modelled in
   *      csrc/dsm_bf16_mfma_model.h (validated on the hardware: experiments/bf16_adder_probe.hip).  Every product is exact; the
   *      matrix pipe does a third of the cycles per k ... at 16 x the rate.
   * The presets below (and config_toml's default) select 1, the mode bench.py times; tests/test_dot_mode_agreement_gpu.py bounds
   * its distance from mode 0 at the real dimensions. */
  int dot_mode;
} dsm_asr_config;

/* Presets matching configs/stt/config-stt-en_fr-hf.toml and config-stt-en-hf.toml. */
void dsm_mimi_config_v0_1(dsm_mimi_config* out, int num_codebooks);
void dsm_asr_config_stt_1b_en_fr(dsm_asr_config* out);
void dsm_asr_config_stt_2_6b_en(dsm_asr_config* out);

typedef struct dsm_engine dsm_engine; /* opaque: one per (device, BatchedAsr module) */

/* AsrMsg — core/asr.rs:9-13.  Word tokens are returned through a side buffer. */
enum { DSM_MSG_STEP = 0, DSM_MSG_WORD = 1, DSM_MSG_END_WORD = 2 };
typedef struct dsm_asr_msg {
  int kind;
  int batch_idx;       /* Word / EndWord */
  int step_idx;        /* Step: model_step_idx after the step */
  double time;         /* Word: start_time, EndWord: stop_time (seconds) */
  int tokens_offset;   /* Word: tokens live in tokens_out[offset .. offset+n_tokens) */
  int n_tokens;
  float prs[DSM_MAX_EXTRA_HEADS]; /* unused here; Step probabilities come from vad_prs_out */
} dsm_asr_msg;

typedef struct dsm_metrics {
  double last_encode_us;     /* device time of the last dsm_mimi_encode_step (HIP events) */
  double last_lm_us;         /* device time of the last dsm_asr_step_tokens */
  double algorithmic_bytes_encode; /* BASELINE.md bytes_step() terms, for roofline.achieved */
  double algorithmic_bytes_lm;
  uint64_t steps_encode;
  uint64_t steps_lm;
  uint64_t graph_launches;   /* launch sequences replayed as one hipGraphLaunch (Mimi encode / decode, one LM stream group, one TTS step) */
  uint64_t eager_bodies;     /* the same sequences enqueued launch by launch (warm-up runs, DSM_GRAPHS=0, profiling on) */
  uint64_t capture_failures; /* stream captures that were begun and did not end in a launchable graph (the body then ran launch by
                                launch; the capture is retried up to three times before that sequence stays eager).  Expected: 0 */
  char capture_error[96];    /* what the FIRST such failure reported (hipGetErrorString / the engine's own reason), "" if none */
} dsm_metrics;

/*
 * Create.  Replaces LmModel::batched + Mimi::batched + asr::State::new
 * (srv/batched_asr.rs:738-758, 272-278; core/lm.rs:816; core/mimi.rs:113; core/asr.rs:65).
 * Reads the same safetensors keys as the reference; LM tensors must be
 * BF16 or F32 (stored as bf16 on device), Mimi tensors F32/BF16 (stored as f32,
 * core/mimi.rs:250-255).  Fails with DSM_ERR_DEVICE if no gfx950 device is usable — there
 * is no CPU fallback in this library.
 */
int dsm_asr_create(const dsm_asr_config* cfg, int device_id, int batch_size,
                   const char* lm_safetensors, const char* mimi_safetensors, dsm_engine** out);
void dsm_destroy(dsm_engine*);
const char* dsm_last_error(const dsm_engine*); /* NULL engine -> last create error */

/*
 * Multi-GPU load (the reference is single-device: srv/main.rs:317-327).  Every immutable weight
 * tensor of an engine lives in ONE contiguous device allocation (the "weight arena": packed bf16 LM matrices, f32 Mimi
 * matrices, folded codebooks, norms — 2.0 GB for stt-1b-en_fr), carved in load order.  The rank that read the
 * safetensors exposes it with dsm_asr_weight_arena; the launcher broadcasts those bytes once (RCCL over xGMI: the only
 * collective of the whole path) together with the small manifest (the answers of the loader's optional-key probes, one
 * byte each), and every other rank attaches with dsm_asr_create_from_arena: no file, no conversion, no packing, no
 * host copy.  The arena handed to dsm_asr_create_from_arena stays owned by the caller and must outlive the engine; it
 * must sit on device `device_id`.  Configuration and batch size may differ per rank only in batch_size.
 */
int dsm_asr_weight_arena(dsm_engine*, void** d_arena, size_t* arena_bytes, const uint8_t** manifest, size_t* manifest_bytes);
int dsm_asr_create_from_arena(const dsm_asr_config* cfg, int device_id, int batch_size, const void* d_arena,
                              size_t arena_bytes, const uint8_t* manifest, size_t manifest_bytes, dsm_engine** out);
/* r04 — one process, several devices (the reference is one process: srv/main.rs:317-327): a second engine on `device_id` whose
 * weights are a device-to-device copy of `src`'s arena (hipMemcpyPeerAsync over xGMI in 256 MB pieces; a plain device copy when
 * device_id is src's own device).  The replica owns its copy; `cfg` NULL = src's configuration.  INTEGRATION.md shows the Rust
 * server creating one engine + one worker per GPU this way and routing a new socket to the first worker with a free slot. */
int dsm_asr_create_replica(dsm_engine* src, const dsm_asr_config* cfg, int device_id, int batch_size, dsm_engine** out);

/*
 * Mimi::encode_step(&StreamTensor, &StreamMask) — core/mimi.rs:195-206, called at
 * srv/batched_asr.rs:362 (encoder thread).  pcm: host [B*1920] f32; mask: host [B] u8;
 * codes_out: host [B*n_q] u32 (slot-major, [B, n_q, 1] like the reference) or NULL to keep
 * the codes on the device for a following dsm_asr_step_tokens(codes == NULL).
 * *produced = number of frames emitted (always 1 for 1920-sample frames).
 * Codes of inactive slots are unspecified (the reference computes garbage for them and
 * ignores it: core/asr.rs:177-183).
 */
int dsm_mimi_encode_step(dsm_engine*, const float* pcm, const uint8_t* mask, uint32_t* codes_out,
                         int* produced);

/*
 * Mimi::decode_step(&StreamTensor codes [B,n_q,1], &StreamMask) — core/mimi.rs:217-225 (called by the TTS worker at
 * srv/tts.rs:538): quantizer decode -> ConvTr upsample -> decoder transformer -> SEANet decoder.
 * codes: host [B*n_q] u32 (values < quantizer_bins); pcm_out: host [B*1920] f32.  *produced = samples per slot.
 * The decode state is allocated on first use and belongs to the encoder-side Mimi (dsm_mimi_reset_slot resets its conv
 * carries; like the reference it does NOT reset the decoder transformer: core/mimi.rs:237-238).
 */
int dsm_mimi_decode_step(dsm_engine*, const uint32_t* codes, const uint8_t* mask, float* pcm_out, int* produced);
int dsm_mimi_decode_step_dev(dsm_engine*, const uint32_t* d_codes, const uint8_t* d_mask, float* d_pcm_out);

/*
 * asr::State::step_tokens(&Tensor[B,n_q,1], None, &StreamMask, f) — core/asr.rs:147-255,
 * called at srv/batched_asr.rs:476 (model thread).  codes: host [B*n_q] u32 or NULL (use the
 * device-resident output of the last encode step).  text_tokens_out: host [B] u32 (argmax
 * per slot, valid for active slots).  vad_prs_out: host [extra_heads_num*B] f32 (class-0
 * probability of every extra head, layout [head][slot], core/asr.rs:195-203) or NULL.
 * Word/EndWord/Step messages produced by this step are queued for dsm_asr_poll_msgs.
 */
int dsm_asr_step_tokens(dsm_engine*, const uint32_t* codes, const uint8_t* mask,
                        uint32_t* text_tokens_out, float* vad_prs_out);

/* asr::State::step_pcm — core/asr.rs:115-131 (warmup path, srv/batched_asr.rs:236):
 * encode_step on the MODEL side's own Mimi state followed by step_tokens. */
int dsm_asr_step_pcm(dsm_engine*, const float* pcm, const uint8_t* mask, uint32_t* codes_out,
                     uint32_t* text_tokens_out, float* vad_prs_out);

/* The same two calls for callers that run the reference's thread pair with run-ahead (encoder_loop feeds model_loop through a
 * bounded channel, srv/batched_asr.rs:291,314-522): dsm_mimi_encode_step_async copies the frame, enqueues upload + encode on the
 * encoder stream and returns at once with a ticket (ring of 4 frames: DSM_ERR_STATE while all four wait for the model side);
 * dsm_asr_step_tokens_ticket makes the model stream wait for that frame's codes (kept in a per-ticket device copy), runs the
 * LM step and returns tokens like dsm_asr_step_tokens.  Encode of frame n+1 then overlaps the LM step of frame n on the GPU.
 * Tickets must be consumed in the order they were issued. */
int dsm_mimi_encode_step_async(dsm_engine*, const float* pcm, const uint8_t* mask, int* ticket);
int dsm_asr_step_tokens_ticket(dsm_engine*, int ticket, const uint8_t* mask, uint32_t* text_tokens_out, float* vad_prs_out);

/* Read the Vec<AsrMsg> the last step returned (the list lives until the next step: polling does not consume it).
 * Returns the number of messages written (<= cap; a step yields at most 2*B + 1); word tokens are copied to
 * tokens_out, truncated to tokens_cap entries — a Word whose tokens_offset + n_tokens exceeds tokens_cap was cut:
 * poll again with a larger buffer (dsm_worker_step does exactly that). */
int dsm_asr_poll_msgs(dsm_engine*, dsm_asr_msg* msgs, int cap, uint32_t* tokens_out, int tokens_cap);

/* ---- token scores: how sure the model was (this project's own; the reference keeps the argmax and drops the logits row,
 * core/asr.rs:208-215).  Off by default: a step then enqueues exactly what it enqueues without this section.
 * Definition (csrc/dsm_token_scores.h, bit-identical on host and device): over the raw text logits of a slot, at softmax
 * temperature 1 — also when cfg.temperature > 0 drew the token with Gumbel noise, where top_ids[0] may differ from the token —
 *   logprob     log softmax of the step's text token,
 *   top_n best  the first top_n entries of the row by value descending, then id ascending: id and logprob each; entries beyond
 *               the vocabulary are id 0xFFFFFFFF, logprob -inf.
 * Rows of inactive slots are unspecified, like their text token.
 *   dsm_asr_set_token_scores  top_n = -1 turns scores off, 0 .. DSM_SCORES_MAX_TOP on with that many alternatives;
 *     DSM_ERR_INVALID otherwise.  Any time between steps; waits for calls in progress on other threads.  A change of the setting
 *     makes the LM step's graphs settle again (two eager steps), it is not a per-step switch.
 *   dsm_asr_token_scores      the scores of the last dsm_asr_step_tokens / _step_pcm / _step_tokens_ticket (which bring them to the
 *     host with the tokens): logprob_out [B], top_ids_out / top_logprobs_out [B][top_n] or NULL.  Returns top_n.  DSM_ERR_STATE
 *     while scores are off, or before the first such step since the setting changed.
 *   dsm_asr_token_scores_dev  for the *_dev callers: the engine's device buffers, valid after dsm_sync and overwritten by the next
 *     step; logprob [B], the two top buffers [B][DSM_SCORES_MAX_TOP] (row stride DSM_SCORES_MAX_TOP whatever top_n).  Returns top_n.
 *   dsm_asr_poll_word_scores  parallel to the tokens_out of dsm_asr_poll_msgs: entry msg.tokens_offset + i is the logprob of that
 *     Word's token i; NaN = not recorded (the token came while scores were off, or with an imported snapshot).  Returns the
 *     number of floats written (<= cap).  DSM_ERR_STATE while scores are off.
 *   dsm_token_scores_host     host only, no device needed (like dsm_slot_blob_info): the definition computed serially for one
 *     row of V logits and a token.  DSM_ERR_INVALID for V < 1, token >= V, top_n outside 0 .. DSM_SCORES_MAX_TOP, or a NULL
 *     pointer that is needed (top_ids / top_logprobs may be NULL when top_n is 0).
 *   dsm_debug_token_scores    test aid: runs the step's KERNEL on caller-supplied rows — host logits [n][V] and tokens [n] in,
 *     host logprob_out [n], top_ids_out / top_logprobs_out [n][top_n] out.  Synchronises the model stream. */
#define DSM_SCORES_MAX_TOP 8
int dsm_asr_set_token_scores(dsm_engine*, int top_n);
int dsm_asr_token_scores(dsm_engine*, float* logprob_out /*[B]*/, uint32_t* top_ids_out /*[B][top_n] or NULL*/,
                         float* top_logprobs_out /*[B][top_n] or NULL*/);
int dsm_asr_token_scores_dev(dsm_engine*, const float** d_logprob, const uint32_t** d_top_ids, const float** d_top_logprobs);
int dsm_asr_poll_word_scores(dsm_engine*, float* logprobs_out, int cap);
int dsm_token_scores_host(const float* logits, int V, uint32_t token, int top_n, float* logprob, uint32_t* top_ids,
                          float* top_logprobs);
int dsm_debug_token_scores(dsm_engine*, const float* logits, int n, int V, const uint32_t* tokens, int top_n,
                           float* logprob_out, uint32_t* top_ids_out, float* top_logprobs_out);

/* asr::State::reset_batch_idx(slot) — core/asr.rs:257-266, srv/batched_asr.rs:467-471.
 * Resets the LM slot (KV index/position, item state) and the MODEL side's Mimi slot.
 * The reference never resets the ENCODER thread's Mimi clone;
 * dsm_mimi_reset_slot exposes that missing reset explicitly instead of hiding a
 * behaviour change inside dsm_asr_reset_slot. */
int dsm_asr_reset_slot(dsm_engine*, int slot);
int dsm_mimi_reset_slot(dsm_engine*, int slot);
/* temperature > 0 only: (re)start the slot's Gumbel-noise stream at word 0 of ChaCha12 keyed by rand's seed_from_u64(seed)
 * (slot b starts with seed 0x5EED0000 + b).  A reset of the slot does not touch the stream, like the reference's global generator. */
int dsm_asr_set_seed(dsm_engine*, int slot, uint64_t seed);

/* ---- slot snapshots: export, import and move a stream's state (this project's own; the reference is one process on one
 * device and has no such call).  A snapshot holds everything a step of slot s reads that an earlier step of slot s wrote:
 *   LM       the K / V ring rows of every layer, ring position and write index, first_step, the fed-back text token, the
 *            one-step-shifted audio codes, the Gumbel stream's key and position;
 *   Mimi     for the encoder-thread side always, for the model side once it exists (first dsm_asr_step_pcm[_dev]): the encoder
 *            transformer's ring rows with position and index, and every carried conv state (the downsample conv's left pad too);
 *   host     the word-assembly item (step index, pending word tokens, unended_word, last stop time).
 * NOT in a snapshot: the Mimi DECODE state (dsm_mimi_decode_step), the activation scratch and anything else a step overwrites
 * before it reads, the worker's channels (dsm_worker), captured graphs, metrics, and the TTS engine (whose blob format, not yet its calls, is dsm_tts_slot_blob_info below).
 * Nor the token scores (dsm_asr_set_token_scores): neither the setting nor the scores of a pending word's tokens — after an import
 * or a move those read NaN in dsm_asr_poll_word_scores, tokens that arrive later carry real scores, and the blob's bytes do not
 * depend on whether the exporter had scores on.
 * After an import the stream continues bit for bit — codes, tokens, VAD, words — as if it had stayed where it was.  One
 * exception, stated: a slot exported from a Mimi side that has never stepped and imported into a side that has behaves like a
 * reset slot there (zero left pad) — the module-level first call that would have replicated its first frame cannot be moved.
 * The blob (csrc/dsm_slot_blob.h) carries a signature of every configuration field that fixes a size or a
 * meaning; batch size, dot_mode and the device may differ between exporter and importer.
 *   dsm_asr_export_slots  waits for everything enqueued on the engine, packs the n slots with one kernel launch and copies the
 *     blob to `buf`.  *needed (optional) receives the blob's size; buf NULL: size query only; cap < size: DSM_ERR_INVALID.
 *     DSM_ERR_STATE while a dsm_mimi_encode_step_async ticket is outstanding.  The source slots are left untouched — the
 *     caller resets them (dsm_asr_reset_slot + dsm_mimi_reset_slot) before reuse.
 *   dsm_asr_import_slots  slot i of the blob goes to slots[i].  Everything is validated before anything is written:
 *     DSM_ERR_INVALID — engine unchanged, dsm_last_error names the first mismatch — for a different signature, a truncated or
 *     malformed blob, n different from the blob's, a slot out of range or listed twice, or an index-valued field out of range
 *     (ring index >= context, text token / audio code outside its vocabulary, Gumbel position not a multiple of 16).  A blob
 *     with the model-side Mimi brings that side into being here; one without resets that side of the slot.  Works on an
 *     engine that has never stepped: the other slots then behave exactly as in a fresh engine.
 *   dsm_asr_move_slots    src_slots[i] of src -> dst_slots[i] of dst on the SAME device (DSM_ERR_DEVICE otherwise: across
 *     devices, export then import), through a device staging buffer, no host copy.  src == dst with disjoint lists forks a
 *     stream.  Duplicate destination slots: DSM_ERR_INVALID.  Errors are reported on src (dsm_last_error(src)).
 *   dsm_slot_blob_info    host only, no device needed: checks header and host section, fills *out. */
#define DSM_SLOT_BLOB_HAS_MODEL_MIMI 1u
#define DSM_SLOT_SIDE_PRISTINE0 1u
struct dsm_slot_blob_info { /* no typedef: the function below has the name (struct tags are a namespace of their own in C) */
  uint32_t version, n_slots, flags, sig_words;
  uint64_t host_bytes, slot_bytes, total_bytes; /* host section, device payload per slot, the whole blob */
};
int dsm_asr_export_slots(dsm_engine*, const int* slots, int n, void* buf, size_t cap, size_t* needed);
int dsm_asr_import_slots(dsm_engine*, const int* slots, int n, const void* buf, size_t len);
int dsm_asr_move_slots(dsm_engine* src, const int* src_slots, dsm_engine* dst, const int* dst_slots, int n);
int dsm_slot_blob_info(const void* buf, size_t len, struct dsm_slot_blob_info* out);

/* Device::synchronize — srv/batched_asr.rs:238. */
int dsm_sync(dsm_engine*);

int dsm_get_metrics(dsm_engine*, dsm_metrics* out);
int dsm_batch_size(const dsm_engine*);
int dsm_n_q(const dsm_engine*); /* mimi.config().quantizer_n_q — srv/batched_asr.rs:379 */

/*
 * Device-resident variants for callers that already hold HBM buffers (bench.py's timed
 * region; a Rust caller with hipMalloc'd staging).  Pointers are DEVICE pointers, nothing
 * is synchronised; work is enqueued on the engine's encoder / model / group streams, which are
 * NON-BLOCKING: they are not ordered against the null stream or the caller's streams.  The caller
 * makes its inputs visible before the call (stream/device synchronise after filling them) and
 * reads outputs only after dsm_sync; inputs must stay unmodified until then.
 */
int dsm_mimi_encode_step_dev(dsm_engine*, const float* d_pcm, const uint8_t* d_mask, uint32_t* d_codes_out);
int dsm_asr_step_tokens_dev(dsm_engine*, const uint32_t* d_codes, const uint8_t* d_mask,
                            uint32_t* d_text_tokens_out, float* d_vad_prs_out);
/* Make the model stream wait for everything enqueued so far on the encoder stream. */
int dsm_streams_join(dsm_engine*);
/* step_pcm with device pointers: Mimi encode (model-side state) + LM step, all enqueued on the
 * model stream, nothing synchronised.  d_codes_out / d_text_tokens_out / d_vad_prs_out may be NULL. */
int dsm_asr_step_pcm_dev(dsm_engine*, const float* d_pcm, const uint8_t* d_mask, uint32_t* d_codes_out,
                         uint32_t* d_text_tokens_out, float* d_vad_prs_out);

/* Per-kernel-class device timing with HIP events recorded on the stream each kernel is launched on
 * (feeds bench.py's roofline object).  tag_mask selects classes; dsm_prof_read synchronises, adds
 * up the elapsed time of every bracketed launch since the last read, and resets. */
enum { DSM_PROF_ATTN_LM = 0, DSM_PROF_GEMM_LM = 1, DSM_PROF_ATTN_MIMI = 2, DSM_PROF_GEMM_MIMI = 3,
       DSM_PROF_RVQ = 4, DSM_PROF_OTHER = 5, DSM_PROF_NTAGS = 6 };
int dsm_prof_enable(dsm_engine*, unsigned tag_mask);
int dsm_prof_read(dsm_engine*, double* total_us /*[DSM_PROF_NTAGS]*/, uint64_t* launches /*[DSM_PROF_NTAGS]*/);
/* Same classes, but bracketed INSIDE the kernel with the device wall clock (first workgroup in, last workgroup out):
 * the duration rocprofv3's kernel trace reports.  With several streams in flight a HIP-event bracket also counts the
 * time a launch queues behind other streams' kernels.  Instrumented classes: ATTN_LM, ATTN_MIMI (others read 0). */
int dsm_prof_read_device(dsm_engine*, double* total_us /*[DSM_PROF_NTAGS]*/, uint64_t* launches /*[DSM_PROF_NTAGS]*/);
/* Timeline diagnostics (tools/timeline.py): with `on`, the tiled GEMM launches and their reduce launches are bracketed in the
 * kernel like the attention launches; dsm_prof_timeline_read returns every bracketed launch since the last read as (stream id:
 * 0 encoder, 1 + g LM group g; kind: 0 attention, 1 GEMM, 2 reduce; class tag; start / end in us from the earliest start). */
int dsm_prof_timeline(dsm_engine*, int on);
int dsm_prof_timeline_read(dsm_engine*, int* sid, int* kind, int* tag, double* start_us, double* end_us, int cap);

/* ------------------------------------------------------------------------------------------------
 * TTS (BASELINE.json configs[4]): tts_streaming::State::step + LmModel::forward_cond + DepFormer::sample
 * (core/tts_streaming.rs:117-242, core/lm.rs:957-1008, :640-684); Sampling::ArgMax by default (what the reference
 * selects when temperature <= 0, srv/tts.rs:402), seeded top-k per slot with dsm_tts_set_sampling.  The reference serves one generation at a
 * time behind a mutex (srv/tts.rs:374); here B independent generations advance together, each slot with its
 * own step index (batching the TTS path is new capability).
 * ------------------------------------------------------------------------------------------------ */
#define DSM_TTS_UNGENERATED 0xFFFFFFFFu /* tts_streaming::UNGENERATED */
enum { DSM_TTS_ALLOW_PAD = -1, DSM_TTS_ALLOW_PAD_OR_EPAD = -2 }; /* AllowedTokens::{Pad, PadOrEpad}; >= 0: Text(v) */

typedef struct dsm_tts_config {
  dsm_transformer_config lm;        /* [modules.tts.model.transformer] */
  int text_in_vocab_size, text_out_vocab_size, audio_vocab_size, audio_codebooks;
  dsm_transformer_config depformer; /* [modules.tts.model.depformer.transformer]; positional_embedding = None */
  int dep_num_slices;               /* DepFormerConfig::num_slices = generated audio codebooks */
  int dep_low_rank;                 /* low_rank_embeddings (0 = full-rank tables) */
  int dep_weight_groups;            /* distinct linear_in / gating weight sets: idx*groups/num_slices (core/lm.rs:527,558) */
  /* tts_streaming::Config — core/tts_streaming.rs:12-44 */
  int acoustic_delay, text_pad_token, text_bos_token, text_eos_token, text_eop_token, text_start_token;
  int text_audio_delay_in_tokens, max_consecutive_pads, max_steps;
  int kv_bf16;
  /* The branch the reference's TTS server runs (srv/tts.rs:426-441: State::new(.., Some(CaSrc::Tokens(ca_src)), .., cfg_alpha, ..)):
   * cross-attention to a speaker-conditioning source in every main-LM layer (core/lm.rs:392-396 tts_202501:
   * cross_attention = Some((Normal, LayerNorm, None)); core/transformer.rs:205-330,747-763) and classifier-free guidance
   * (core/tts_streaming.rs:164-173,207-214).  All zero = the `ca_src = None`, `cfg_alpha = None` path. */
  int cross_attention;   /* 1: every main-LM layer carries norm_cross + cross_attention.{in_proj_weight_q, in_proj_weight_kv, out_proj}
                            (or the legacy single in_proj_weight); gating must be CrossAttentionGating::Normal */
  int ca_norm;           /* norm_cross: 0 LayerNorm (eps 1e-5, weight|alpha + bias), 1 RmsNorm (eps 1e-8, alpha) — cfg.cross_attention.1 */
  int ca_dim;            /* width of a cross-attention source row (kv_in_dim, cfg.cross_attention.2); 0 = d_model */
  int ca_max_len;        /* longest source (rows of ca_src) a slot may be given with dsm_tts_set_ca_src */
  int cfg_rows;          /* 1: every slot owns TWO batch rows (conditional, unconditional) so that it can run with a cfg_alpha */
  int dot_mode;          /* as dsm_asr_config.dot_mode */
} dsm_tts_config;
void dsm_tts_config_v202501(dsm_tts_config* out); /* Config::v202501 + configs/tts/config-tts.toml with a consistent depformer */

typedef struct dsm_tts dsm_tts;
int dsm_tts_create(const dsm_tts_config* cfg, int device_id, int batch_size, const char* lm_safetensors, dsm_tts** out);
void dsm_tts_destroy(dsm_tts*);
const char* dsm_tts_last_error(const dsm_tts*);
/* State::step for every active slot.  prev_text_token [B]; allowed [B] (>= 0 Text(v), DSM_TTS_ALLOW_*);
 * text_token_out [B]; audio_out [B*num_slices]: this step's last_audio_tokens (depformer samples) or
 * DSM_TTS_UNGENERATED while step_idx < text_audio_delay_in_tokens.  */
int dsm_tts_step(dsm_tts*, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                 uint32_t* text_token_out, uint32_t* audio_out);
/* audio_tokens[step] of a slot (delayed write-back applied, core/tts_streaming.rs:220-236); entries may be UNGENERATED */
int dsm_tts_audio_tokens(dsm_tts*, int slot, int step, uint32_t* out /* [num_slices] */);
int dsm_tts_step_idx(dsm_tts*, int slot);
int dsm_tts_reset_slot(dsm_tts*, int slot);
/* The slot's text and audio LogitsProcessor (srv/tts.rs:401-415): Sampling::TopK{k, temperature} seeded with `seed` when
 * temperature > 0 and top_k > 1, Sampling::ArgMax otherwise (the default after create and after dsm_tts_reset_slot).
 * Softmax over the whole vocabulary at the temperature, the k most probable tokens (probability descending, token id
 * ascending), one weighted draw from a ChaCha12 stream (rand 0.9 StdRng, seed_from_u64): csrc/dsm_sampling.h.  The
 * reference's order among the k survivors is an implementation detail of Rust's select_nth_unstable_by and no vector of
 * candle's / rand's exists offline: sampled tokens are pinned engine-vs-oracle only ("parity unpinned" vs Candle). */
int dsm_tts_set_sampling(dsm_tts*, int slot, int top_k, float temperature, uint64_t seed);
/* The slot's cross-attention source and guidance — the `ca_src` / `cfg_alpha` arguments of tts_streaming::State::new
 * (core/tts_streaming.rs:70-100; built at srv/tts.rs:426-441 from the voice's `ca_src` tensor, with the speaker encoder's
 * empty conditioning appended as a second batch row when the query carries a cfg_alpha).
 *   ca_src [n][ca_dim] f32, host: CaSrc::Tokens of batch row 0.  Its keys and values (in_proj_kv, core/transformer.rs:299-318)
 *     are projected ONCE here into a per-slot device buffer; the reference recomputes the same values every step.
 *     NULL / n = 0: ca_src = None (cross-attention is skipped for the slot: core/transformer.rs:753-760).
 *   ca_src_uncond [n_uncond][ca_dim] or NULL: batch row 1 (needs cfg_rows = 1).  With it the slot runs both rows and mixes
 *     text logits and every depformer slice's logits as l0 * a - l1 * (a - 1), a = cfg_alpha (core/tts_streaming.rs:166-172,
 *     core/lm.rs:718-721: Tensor * f64 = affine(mul as f32, 0)), sampling once per slot.
 * Needs cfg.cross_attention; n, n_uncond <= ca_max_len.  dsm_tts_reset_slot clears both (a fresh State). */
int dsm_tts_set_ca_src(dsm_tts*, int slot, const float* ca_src, int n, const float* ca_src_uncond, int n_uncond, double cfg_alpha);
/* Voices: a source projected ONCE into device memory of its own, which any number of slots attach to by reference.
 * dsm_tts_set_ca_src pays the in_proj_kv projection of every layer for every request and gives every batch row a private copy;
 * a deployment has a handful of voices and one unconditional source for all guided requests.  The reference has no such
 * object: its voice cache (srv/tts.rs:41-60, 702-744, ca_srcs / dynamic_ca_srcs) holds un-projected rows and compute_kv runs
 * on them every step.  A voice holds, bit for bit, what dsm_tts_set_ca_src would have written for the same rows (same GEMM, same
 * scatter kernel, another destination), so a slot computes the same tokens either way.
 *   dsm_tts_voice_create   compute_kv(CaSrc::Tokens(ca_src)) (core/transformer.rs:299-318) for every main-LM layer into
 *     [H][ca_max_len][hd] blocks for K and for V in the cache dtype (kv_bf16).  *voice_out: the handle, > 0 and never reused
 *     during the engine's life (0 = none).  Synchronous, on the model stream between steps, like dsm_tts_set_ca_src /
 *     dsm_tts_encode_voice; a generation in progress is not disturbed.  DSM_ERR_STATE without cfg.cross_attention;
 *     DSM_ERR_INVALID for n < 1, n > ca_max_len or NULL rows; an allocation failure creates nothing and leaves the engine as it was.
 *   dsm_tts_set_voice      the slot's rows read `voice` (batch row 0) and `voice_uncond` (batch row 1; 0 = no guidance) from now
 *     on.  Preconditions and errors of dsm_tts_set_ca_src: a fresh slot (step index 0) unless both are 0, which clears like
 *     NULL rows do; voice_uncond needs cfg_rows = 1 and a conditional voice; cfg_alpha is stored as the same two f32 factors.
 *     DSM_ERR_INVALID for an unknown or destroyed handle.  No GEMM and no copy of K / V: the row's base pointers (one small
 *     table entry per layer), its length and the guidance flag and factors are uploaded.  Replaces whatever the slot had
 *     (private rows or other voices) and counts one reference per batch row that points at a voice.  dsm_tts_set_ca_src (rows
 *     or NULL), dsm_tts_reset_slot and a later dsm_tts_set_voice drop the slot's references.
 *   dsm_tts_voice_destroy  DSM_ERR_STATE ("in use by n rows") while referenced, nothing freed; else waits for the model stream
 *     and frees.  dsm_tts_destroy frees what is left.
 *   dsm_tts_voice_info     rows, current references, device bytes (any of the three may be NULL); DSM_ERR_INVALID for a bad
 *     handle.  The bytes are those of the K / V blocks, 2 * layers * d_model * ca_max_len * element size — what one batch row's
 *     private blocks take — without the 256 bytes of slack every device allocation of the engine carries.
 * Rows attached to one voice read the same addresses, so its K / V are shared in the caches. */
int dsm_tts_voice_create(dsm_tts*, const float* ca_src /* host [n][cond_dim] f32 */, int n, int* voice_out);
int dsm_tts_voice_destroy(dsm_tts*, int voice);
int dsm_tts_voice_info(dsm_tts*, int voice, int* rows, int* refs, size_t* device_bytes);
int dsm_tts_set_voice(dsm_tts*, int slot, int voice, int voice_uncond /* 0 = no guidance */, double cfg_alpha);
/* ---- The TTS slot blob: the container a generation's slot state travels in (csrc/dsm_tts_slot_blob.h; DESIGN.md section 7.2
 * has the table of state it is laid out for and the layout).  Same conventions as the STT blob above — little-endian, 16-byte
 * aligned sections, a signature of every configuration field that fixes a size or a meaning, an importer that never reads an
 * offset from the blob — with a magic of its own: dsm_slot_blob_info and dsm_asr_import_slots refuse a TTS blob with "bad
 * magic", and dsm_tts_slot_blob_info refuses an STT blob the same way.  The engine calls that fill and consume such a blob
 * (export, import, move) are NOT in the library yet: only the format, its writer, its checked reader and the payload's layout are.
 *   dsm_tts_slot_blob_info  host only, no device needed: checks header and host section (every count against its bound, the
 *     sizes against each other and against `len`), fills *out.  DSM_ERR_INVALID with dsm_tts_last_error(NULL) naming the fault.
 *   dsm_tts_slot_layout     host only, no device, pure: the device payload's section list for a configuration (mimi NULL:
 *     without the Mimi decode group) as text, one line per section "name bytes_per_slot payload_offset", then "slot_bytes N"
 *     and "signature w0 w1 ...".  Returns the text's length; the text is written (NUL-terminated) when cap is larger.
 *     DSM_ERR_INVALID, dsm_tts_last_error(NULL), for a configuration no engine can have.  csrc/dsm_tts_slot_layout.h, which
 *     also holds the index checks an import has to make before it writes (tests/sanitize_tts_xfer/ runs them under sanitizers). */
#define DSM_TTS_SLOT_BLOB_HAS_MIMI_DEC 1u
struct dsm_tts_slot_blob_info {
  uint32_t version, n_slots, flags, sig_words, slices /* dep_num_slices */, reserved;
  uint64_t host_bytes, slot_bytes, total_bytes; /* host section, device payload per slot, the whole blob */
};
int dsm_tts_slot_blob_info(const void* buf, size_t len, struct dsm_tts_slot_blob_info* out);
int dsm_tts_slot_layout(const dsm_tts_config*, const dsm_mimi_config* /* NULL: no decode group */, char* buf, size_t cap);
/* Generated frames to PCM — what the reference's TTS worker does with every step's tokens: a second thread receives
 * state.last_audio_tokens() and runs Mimi::decode_step on them (srv/tts.rs:528-544, core/mimi.rs:217-225) while the inference
 * loop is already in its next step.
 *   dsm_tts_attach_mimi   the Mimi for the generated frames (srv/tts.rs:309-310 mimi::load(audio_tokenizer_file,
 *     Some(audio_codebooks))), loaded into this object: no LM checkpoint of an STT engine is involved.  DSM_ERR_INVALID unless
 *     quantizer_n_q == dep_num_slices and quantizer_bins >= audio_vocab_size - 1; DSM_ERR_STATE when the checkpoint has no
 *     decoder.* tensors or a Mimi is attached already.
 *   dsm_tts_step_pcm      State::step (tokens, audio_out, step indices and the dsm_tts_audio_tokens table exactly as dsm_tts_step)
 *     + the audio_processing_loop's decode of the frame this step completed.  With s the slot's step index before the call, a
 *     slot emits iff mask[b], s >= text_audio_delay_in_tokens + acoustic_delay and no token of audio_tokens[s - acoustic_delay]
 *     is >= audio_vocab_size - 1 (last_audio_tokens, core/tts_streaming.rs:275-287, and the test at srv/tts.rs:537): codebook 0
 *     of that row was sampled acoustic_delay steps ago, codebooks >= 1 by this step.  pcm_valid_out[b] is that predicate; the
 *     1920 samples of a slot that did not emit are left alone.  The frame is assembled on the device and decoded on the engine's
 *     second stream.  pcm_out != NULL: the call waits for the decode (serial).  pcm_out == NULL: the decode is only enqueued
 *     and the step's entry (PCM + valid, also when no slot emits) waits in a queue of two, so that the decode of step n overlaps
 *     the LM of step n + 1.  DSM_ERR_STATE, nothing touched: no Mimi attached; a third deferred step while two entries wait;
 *     a serial call while any waits.
 *   dsm_tts_recv_pcm      the oldest waiting entry: 1 = delivered (pcm_out [B*1920] and pcm_valid_out [B] may be NULL), 0 = none.
 *   dsm_tts_pcm_pending   entries waiting (0..2).
 * Every slot decodes as a Mimi of its own, fresh at the slot's first frame and again after dsm_tts_reset_slot — the reference
 * decodes every request with clone() + reset_state() (srv/tts.rs:499-500), never with one batched module: a slot that starts after
 * the batch's first frame gets no carry term in its first frame, and dsm_tts_reset_slot also puts the decoder transformer back
 * to position 0 (dsm_mimi_reset_slot, like Mimi::reset_batch_idx, does not).  Frames queued before a reset are still delivered. */
int dsm_tts_attach_mimi(dsm_tts*, const dsm_mimi_config* mimi, const char* mimi_safetensors);
int dsm_tts_step_pcm(dsm_tts*, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                     uint32_t* text_token_out, uint32_t* audio_out,
                     float* pcm_out /* [B*1920] or NULL = deferred */, uint8_t* pcm_valid_out /* [B] */);
int dsm_tts_recv_pcm(dsm_tts*, float* pcm_out, uint8_t* pcm_valid_out);
int dsm_tts_pcm_pending(dsm_tts*);
/* Voice clips to cross-attention rows — what the reference's server does on every voice-cache miss (srv/tts.rs:702-778,
 * 946-964) before a request's first step.  The rows go to dsm_tts_set_ca_src: ca_src from dsm_tts_encode_voice, ca_src_uncond
 * from dsm_tts_speaker_empty (srv/tts.rs:833-838) — or, to pay the projection once per voice instead of once per request,
 * to dsm_tts_voice_create: the engine then keeps the projected voice on the device and requests attach to it with
 * dsm_tts_set_voice (which voice belongs to which name stays with the caller, like the reference's dynamic_ca_srcs map).
 * cond_dim = ca_dim if non-zero, else lm.d_model.  Rows are f32, the dtype dsm_tts_set_ca_src takes: the reference's final
 * to_dtype(self.dtype) (bf16 on its GPU path) is NOT applied.
 *   dsm_tts_attach_speaker_encoder   SpeakerEncoder::new — core/tts_streaming.rs:346-372, srv/tts.rs:311-333.  The speaker
 *     tokenizer is the Mimi attached with dsm_tts_attach_mimi, as in the shipped configuration (configs/tts/config-tts.toml:17-18
 *     names one file twice).  Reads condition_provider.conditioners.speaker_wavs.{output_proj.weight [cond_dim][dimension],
 *     learnt_padding [1,1,cond_dim]} (BF16 or F32, kept as f32) from lm_safetensors and allocates the clip path's scratch for
 *     clips of up to transformer.context / downsample_stride frames.  DSM_ERR_STATE without a Mimi, without cfg.cross_attention
 *     or when attached already; DSM_ERR_IO for a missing key or a wrong shape; DSM_ERR_INVALID for n_speakers < 1.
 *   dsm_tts_encode_voice   SpeakerEncoder::encode — core/tts_streaming.rs:382-409 on the slices the caller has made
 *     (srv/tts.rs:946-964): every clip is scaled to x * 0.08 / stddev(x), encoded by a whole-clip (non-streaming) Mimi encode
 *     (Mimi::encode_pre_quantize, core/mimi.rs:177-183) and projected.  pcm: host [n_clips][clip_len] at 24 kHz, clips beyond
 *     n_speakers are ignored.  clip_len must be a positive multiple of DSM_FRAME_SIZE with clip_len / DSM_FRAME_SIZE *
 *     downsample_stride <= transformer.context (the shipped 10 s clip: 240 000 samples = 250 positions).  With r = clip_len /
 *     1920 and c = min(n_clips, n_speakers) the result is n_speakers * r rows: c * r projected rows, speaker-major, then
 *     (n_speakers - c) * r copies of learnt_padding; row j of the whole gets add_sin_embeddings' pos_emb[j] (core/tts.rs:94-109).
 *     *rows_out is set whenever the clip shape is valid; DSM_ERR_INVALID for n_clips < 1 ("empty speakers in encode"), a bad
 *     clip_len, cap_rows < rows, or a clip whose standard deviation is zero or not finite (the reference would hand NaNs to the
 *     LM).  Synchronous, on the model stream between steps, like dsm_tts_set_ca_src; a generation in progress is not disturbed.
 *     Tolerance-pinned against the streaming oracle; two calls with the same input return identical bytes.
 *   dsm_tts_speaker_empty  SpeakerEncoder::empty — core/tts_streaming.rs:411-416: n_speakers * 125 rows of learnt_padding +
 *     pos_emb (the 125 is the reference's literal, whatever the clip length).
 * dsm_tts_debug_read taps: "spk.pcm_norm" [c][clip_len], "spk.latent" [c * r][dimension] (encode_pre_quantize transposed) of the
 * last encode; "spk.stats" = {scratch MiB, milliseconds between events around that encode's enqueue, the host's wait for the
 * standard deviations included}; "spk.launches" = {kernel launches of that encode's device side: kernel nodes of a discarded capture}. */
int dsm_tts_attach_speaker_encoder(dsm_tts*, int n_speakers, const char* lm_safetensors);
int dsm_tts_encode_voice(dsm_tts*, const float* pcm /* host [n_clips][clip_len], 24 kHz */, int n_clips, int clip_len,
                         float* ca_src_out /* host [rows][cond_dim] */, int cap_rows, int* rows_out);
int dsm_tts_speaker_empty(dsm_tts*, float* ca_src_out, int cap_rows, int* rows_out);
/* A request's text schedule on the device, K steps per visit — the inference loop of the reference's TTS worker
 * (srv/tts.rs:574-621 with words arriving on a channel, :852-907 over a whole prompt) for B slots at once.  The word queue, the
 * cursor (current word, token_idx, step_past_last_token, last_epad_index), last_text_token, consecutive_pads and the step index
 * of every slot live in device memory; two one-thread-per-slot kernels around each step's groups pick `allowed` and
 * prev_text_token and assemble the input tokens (core/tts_streaming.rs:126-158), then do the loop body behind State::step
 * (srv/tts.rs:596-614).  dsm_tts_run only enqueues; dsm_tts_collect waits once for the whole block and replays its records into
 * the host-side token tables, so dsm_tts_audio_tokens / dsm_tts_step_idx answer as after the same dsm_tts_step calls.
 *   dsm_tts_request_begin       a fresh slot (step index 0: dsm_tts_reset_slot, then dsm_tts_set_ca_src / dsm_tts_set_sampling as
 *     needed) starts a request: last_text_token = text_start_token, current word = the empty word (srv/tts.rs:577), so the
 *     first `allowed` is PadOrEpad.  max_seq_len: the loop's `0..max_seq_len` (srv/tts.rs:580); extra_steps: Config::extra_steps
 *     (srv/tts.rs:572,584) — a per-request argument because dsm_tts_config has no such field.  DSM_ERR_STATE: the slot is not
 *     fresh, has a request already, or a block waits.  DSM_ERR_INVALID: max_seq_len < 1 or extra_steps < 0.
 *   dsm_tts_request_push_words  in_tx.send(Some(word_tokens)) for n_words words: tokens back to back, word_len [n_words] (a word
 *     may be empty).  The caller inserts the bos token into the first word (srv/tts.rs:484-493).  The queue holds max_steps +
 *     acoustic_delay tokens and as many words per request (a request cannot consume more than it has steps).  A push that does
 *     not fit, or one on a closed slot or a slot without a request: DSM_ERR_STATE, nothing changed.  The upload rides the model
 *     stream: it is ordered with the blocks, also with one that waits to be collected.
 *   dsm_tts_request_close       in_tx.send(None) (srv/tts.rs:470): after the last word's end-of-pad the slot runs the tail of
 *     extra_steps + text_audio_delay_in_tokens Pad steps and is DONE.
 *   dsm_tts_run                 n_steps (1..DSM_TTS_RUN_MAX) steps of every slot with a request; enqueue only: no synchronize, no
 *     download.  Before each step a slot in DSM_TTS_REQ_WAITING (end-of-pad seen, next word not pushed, not closed) takes its next
 *     word if one has arrived and sits the step out otherwise — the reference blocks a thread in in_rx.recv() there; then the
 *     termination test: step_past_last_token > extra_steps + text_audio_delay_in_tokens (DONE), max_seq_len steps done or the step
 *     that would reach the engine's "max step-idx" (DONE_LIMIT).  decode = 1 (needs dsm_tts_attach_mimi and an empty PCM queue)
 *     also decodes the frame every step completes, with dsm_tts_step_pcm's predicate, each step into a frame buffer and a pinned
 *     PCM entry of its own.  DSM_ERR_STATE, nothing touched: a block waits for dsm_tts_collect; n_steps out of range; decode
 *     without a Mimi.  While a block waits, dsm_tts_step / dsm_tts_step_pcm / dsm_tts_reset_slot return DSM_ERR_STATE; between
 *     blocks dsm_tts_step* serves the other slots (mask[b] = 1 on a slot with a request: DSM_ERR_STATE).
 *   dsm_tts_collect             waits for the block and fills `out` (every array is the caller's, sized for the n_steps given to
 *     dsm_tts_run; any may be NULL).  A slot's text_token / audio entries are defined where stepped is 1 (audio: this step's
 *     last_audio_tokens, or DSM_TTS_UNGENERATED below text_audio_delay_in_tokens).  Word events (srv/tts.rs:596-604) carry steps;
 *     their text is dsm_tts_word_text: word = push-order index (-1: the initial empty word), start_step = last_epad_index, stop_step = the slot's step
 *     index before the step; seconds = step / 12.5.  n_events counts all of them, the first events_cap are stored.
 *     overwrite_last_text_token(pad) (srv/tts.rs:609) is applied to the host's text-token table only; the token handed to the
 *     next step stays the end-of-pad.  DSM_ERR_STATE when no block waits.
 *   dsm_tts_request_status      DSM_TTS_REQ_* as of the last collect (RUNNING right after begin).  dsm_tts_reset_slot ends a
 *     request: the slot is IDLE again. */
#define DSM_TTS_RUN_MAX 16 /* steps per block: one frame buffer and one pinned PCM entry each (16 * B * 1920 * 4 bytes: 3.9 MB at B = 32) */
enum { DSM_TTS_REQ_IDLE = 0, DSM_TTS_REQ_RUNNING = 1, DSM_TTS_REQ_WAITING = 2, DSM_TTS_REQ_DONE = 3, DSM_TTS_REQ_DONE_LIMIT = 4 };
typedef struct dsm_tts_word_event { int slot, word, start_step, stop_step; } dsm_tts_word_event;
typedef struct dsm_tts_block {
  int n_steps;              /* out: steps of the block */
  uint8_t* stepped;         /* [n][B] the slot took this step */
  uint32_t* text_token;     /* [n][B] */
  uint32_t* audio;          /* [n][B][num_slices] */
  float* pcm;               /* [n][B][1920] or NULL; written where pcm_valid is 1 */
  uint8_t* pcm_valid;       /* [n][B] or NULL */
  dsm_tts_word_event* events;
  int events_cap, n_events; /* in, out */
  int* status;              /* [B] DSM_TTS_REQ_* after the block */
} dsm_tts_block;
int dsm_tts_request_begin(dsm_tts*, int slot, int max_seq_len, int extra_steps);
int dsm_tts_request_push_words(dsm_tts*, int slot, const uint32_t* tokens, const int* word_len, int n_words);
int dsm_tts_request_close(dsm_tts*, int slot);
int dsm_tts_run(dsm_tts*, int n_steps, int decode);
int dsm_tts_collect(dsm_tts*, dsm_tts_block* out);
int dsm_tts_request_status(dsm_tts*, int slot);
/* Text in, text out — the two ends of the request loop that the reference's server does with its text_tokenizer:
 *   dsm_tts_attach_tokenizer    once after create.  DSM_ERR_IO / DSM_ERR_INVALID as dsm_spm_load; DSM_ERR_INVALID when the
 *     model has more pieces than text_out_vocab_size; DSM_ERR_STATE when attached already.
 *   dsm_tts_request_push_text   recv_loop's body for one text message (srv/tts.rs:480-494): split on U+0020 only, skip empty
 *     words, encode each word on its own, text_bos_token in front of the first word the request receives — by this call or by
 *     dsm_tts_request_push_words, whose caller inserts its own bos; "first" is per request (dsm_tts_request_begin resets it) —
 *     then the queue upload of dsm_tts_request_push_words.  *n_words (may be NULL) = words queued.  All or nothing:
 *     DSM_ERR_STATE with the queue and the first-word flag unchanged when the words do not fit, the slot is closed or has no
 *     request, or no tokenizer is attached.
 *   dsm_tts_word_text           WordWithTimestamps.text of word event `word` (srv/tts.rs:598): dsm_spm_decode of that word's
 *     tokens as pushed, by either call (the bos decodes to nothing; word -1, the initial empty word, is "").  Returns the byte
 *     length, and the needed one with nothing written when it exceeds cap.  The request's word tokens stay on the host until
 *     dsm_tts_reset_slot; the queue's capacity bounds them.  DSM_ERR_STATE: no tokenizer, no request on the slot;
 *     DSM_ERR_INVALID: no such word, or a pushed token outside the model. */
int dsm_tts_attach_tokenizer(dsm_tts*, const char* path);
int dsm_tts_request_push_text(dsm_tts*, int slot, const char* utf8, size_t len, int* n_words);
int64_t dsm_tts_word_text(dsm_tts*, int slot, int word, char* out, size_t cap);
/* Conditioners — ConditionProvider (core/conditioner.rs:31-176).  The reference's server builds one Condition::AddToInput per
 * request (srv/tts.rs:416-423: condition_lut) and hands it to every State::step; LmModel::forward_cond / forward_ca add it to the
 * input embedding sum of every batch row (core/lm.rs:996-1000, :1062-1066).  Here a slot carries at most one condition: its row
 * [d_model] is computed on the device when it is set (one f32 fma chain per element over k ascending; a continuous value's sin
 * embedding is rounded to bf16 first, like the reference's to_dtype) and is added last in the step's input sum, to both rows of
 * a slot with cfg_rows.  The row stays f32: the reference's final rounding of the projected row to the checkpoint dtype is NOT
 * applied, as for the speaker rows.  A slot without a condition computes exactly what an engine without conditioners computes.
 *   dsm_tts_attach_conditioners    ConditionProvider::new.  Reads condition_provider.conditioners.<name>.{embed.weight
 *     [n_bins + 1][dim] (LUT only), output_proj.weight [d_model][dim], learnt_padding [1,1,d_model]} (BF16 or F32, kept as f32)
 *     from lm_safetensors.  Once per engine, at any time (captured graphs stay valid).  DSM_ERR_IO for a missing key or a wrong
 *     shape (the engine is left as it was), DSM_ERR_INVALID for a bad descriptor, DSM_ERR_STATE when attached already.
 *   dsm_tts_set_condition_lut / _cont / _padding   condition_lut, condition_cont, learnt_padding; a later call replaces the
 *     slot's condition.  Only on a fresh slot (step index 0, no block waiting), like dsm_tts_set_ca_src: DSM_ERR_STATE otherwise,
 *     nothing touched.  DSM_ERR_INVALID: no conditioners attached, an unknown name, a LUT value that is not listed, a string for
 *     a continuous conditioner or a number for a LUT.  A condition set before dsm_tts_request_begin applies to the request.
 *   dsm_tts_clear_condition        always allowed; dsm_tts_reset_slot clears too (a fresh State).
 * dsm_tts_debug_read taps: "cond.row" [B][d_model] (zeros for a slot without a condition), "lm.input" [rows][d_model]: the
 * input sums of the last step. */
enum { DSM_TTS_COND_LUT = 0, DSM_TTS_COND_CONTINUOUS = 1 };
typedef struct dsm_tts_conditioner_desc {
  const char* name;                     /* key under condition_provider.conditioners. */
  int type, dim;
  int n_bins;                           /* LUT: embed.weight is [n_bins + 1][dim] */
  const char* const* possible_values;   /* LUT: value -> its position in this list */
  int n_values;
  float scale_factor, max_period;       /* continuous */
} dsm_tts_conditioner_desc;
int dsm_tts_attach_conditioners(dsm_tts*, const dsm_tts_conditioner_desc*, int n, const char* lm_safetensors);
int dsm_tts_set_condition_lut(dsm_tts*, int slot, const char* name, const char* value);   /* condition_lut */
int dsm_tts_set_condition_cont(dsm_tts*, int slot, const char* name, float value);        /* condition_cont */
int dsm_tts_set_condition_padding(dsm_tts*, int slot, const char* name);                  /* learnt_padding */
int dsm_tts_clear_condition(dsm_tts*, int slot);
int dsm_tts_debug_read(dsm_tts*, const char* name, float* out, size_t cap); /* "lm.hidden", "lm.logits", "lm.input": one row per BATCH ROW (2 per slot with cfg_rows) */
int dsm_tts_get_metrics(dsm_tts*, dsm_metrics* out); /* graph_launches / eager_bodies only */

/* The LM step splits the batch into stream groups (slots [first, first+n) each on its own HIP stream) so that one
 * group's HBM-bound attention overlaps another's MFMA-bound GEMMs; results do not depend on the split.  Returns the
 * number of groups and fills up to `cap` entries.  Environment DSM_LM_GROUPS (1..4) overrides the default at create. */
int dsm_lm_stream_groups(dsm_engine*, int* first_slot, int* n_slots, int cap);
/* Profiling aid: run every group on the model stream, one after the other (per-kernel timings without overlap). */
int dsm_debug_serialize_groups(dsm_engine*, int on);

/* Profiling aid: pretend every slot already streamed `pos` frames (ring index = pos mod ctx, cache content
 * untouched) so that short profiler runs see steady-state attention traffic.  Never used for `value`. */
int dsm_debug_set_positions(dsm_engine*, uint32_t lm_pos, uint32_t mimi_pos);

/* Test aid (teacher forcing): overwrite the text token every slot feeds back into its next step (core/asr.rs:147-160, the
 * `text_token` of State) with `tokens` [batch].  tests/test_dot_mode_agreement_gpu.py drives a dot_mode 1 engine along a
 * dot_mode 0 engine's token history with it, so that one flipped argmax does not cascade. */
int dsm_debug_set_text_tokens(dsm_engine*, const uint32_t* tokens);

/* Debug taps for the parity tests: copy a named intermediate of the last step to the host.
 * Names: "lm.hidden" [B,d], "lm.logits" [B,V], "mimi.seanet_out" [B,T,dim], "mimi.latent" [B,dim] ...
 * Returns the number of floats written, or <0. */
int dsm_debug_read(dsm_engine*, const char* name, float* out, size_t cap);

/* Diagnostic, no device needed: which kernel a matrix product gets.  Runs the GEMM launcher's decision (plan_gemm,
 * csrc/dsm_gemm_plan.h) for an engine kind (stt: the STT engine's defaults, else the TTS engine's) and dot_mode with no DSM_*
 * variable set, for a weight of [N][K] (bf16 or f32), an epilogue (0 store, 1 QKV, 2 gate with N = the hidden width, 3 RVQ),
 * nt n-tiles per wave (2 for the gate, else 1) and M activation rows, and writes one line to buf, e.g.
 *   "bx3u<2> grid=32x4x2 wg=256 lds=49152 chunks=4 loop=0 reduce=rows2 norm=fused mt=2 ... ws=1048576"
 * (kernel form<16-row tiles per workgroup>, grid, workgroup size, dynamic LDS bytes, K-chunks across workgroups, K-chunks
 * walked inside one, the reduce launch: none / consumer / rows1|2|4 / tiles, the row norm: none / fused / separate, then the
 * launcher-owned GemmArgs fields and the split-K workspace bytes).  flags: DSM_GEMMQ_* below.  Returns the line's length, or <0. */
enum {
  DSM_GEMMQ_ALIGNED = 1 << 0,   /* every activation row starts on a multiple of 4 floats */
  DSM_GEMMQ_Y = 1 << 1,         /* an output Y, a second (ELU) output Y2, a residual, a bias, a row norm behind the product */
  DSM_GEMMQ_Y2 = 1 << 2,
  DSM_GEMMQ_RES = 1 << 3,
  DSM_GEMMQ_BIAS = 1 << 4,
  DSM_GEMMQ_NORM = 1 << 5,
  DSM_GEMMQ_Y_OK4 = 1 << 6,     /* the row strides of Y / Y2 / the residual are multiples of 4 floats */
  DSM_GEMMQ_Y2_OK4 = 1 << 7,
  DSM_GEMMQ_RES_OK4 = 1 << 8,
  DSM_GEMMQ_Y_PLAIN = 1 << 9,   /* Y is one plain [M][ld] matrix (no per-batch stride) */
  DSM_GEMMQ_MAY_DEFER = 1 << 10 /* the caller's next kernel can sum split-K slabs itself */
};
int dsm_debug_gemm_plan(int stt, int dot_mode, int weight_bf16, int epi, int nt, int M, int N, int K, int flags, char* buf, size_t cap);
/* The same with the five numbers the decision reads given one by one: knobs = {dot_mode, chunk_loop_min_tiles, smallk_min_tiles,
 * smallk_mt, loop_depth} (GemmKnobs, csrc/dsm_gemm_plan.h); an entry of -1 takes what an engine of the given kind starts from
 * (for dot_mode: 0).  What dsm_debug_gemm below will run for the same shape, flags and knobs. */
int dsm_debug_gemm_plan_knobs(int stt, const int* knobs, int weight_bf16, int epi, int nt, int M, int N, int K, int flags, char* buf, size_t cap);

/* TEST AID, not a serving call: one matrix product through the engine's own GEMM launcher (launch_gemm), on the model stream,
 * eagerly, outside any graph — so that every kernel form the launcher can choose is run alone against a reference
 * (tests/test_gemm_kernels_gpu.py).  Y = epilogue(X W^T) for M rows of X, a weight W [N][K] in f32 on the host (the gate:
 * [2 N][K], gate rows first, N = the hidden width) that is packed the way a checkpoint's weights are (bf16 weights rounded and
 * fragment-major, the gate with its split row), into plain device memory that is released before the call returns — never into
 * the weight arena.  Row r of a matrix starts at element (r / rpb) * bstride + (r % rpb + toff) * ld of its buffer, as in the
 * engine (RowMap): overlapping rows (a convolution over its concat buffer: K > ld), an offset into a concat buffer and rows off
 * a 16-byte boundary can all be said.  Every buffer is copied to the device whole, and Y, Y2 and norm_out are copied back whole:
 * what the caller put outside the M x N result must still be there.
 *   epi       0 store: bias, act (1 = gelu_erf), LayerScale `scale`, residual `res`, Y and / or its ELU copy Y2, a row norm of Y
 *             (norm_w, norm_b unless norm_rms, norm_out [M][N]; Y is then a plain [M][N] matrix and N % 4 == 0);
 *             2 gate: Y = silu(g) * u, nothing else;
 *             1 QKV: offered only where the plan leaves the split-K slabs to the consumer (may_defer), see below — the direct
 *             QKV epilogue (RoPE + ring scatter) and the RVQ epilogue (3) are refused: the model tests keep those.
 *   may_defer the caller could sum split-K slabs itself.  Where the plan then says reduce=consumer the aid sums the slabs with the
 *             library's own ordered slab sum into Y: a plain [M][N] product.
 *   knobs     as for dsm_debug_gemm_plan_knobs, -1 = the engine's own; set for this call and restored after it.
 *   x_back / res_back (optional, x_len / res_len floats): the device copies of X / res after the run; w_changed: 1 when the
 *             packed weight on the device is not what it was before the launch.
 * Also refused: a plan with more than 64 KB of dynamic LDS (the generic kernel at K > 16384) — the launcher never raises a GEMM
 * kernel's dynamic-LDS limit and no engine has such a product, so that launch has never been run.
 * plan receives the line of the plan that ran (as dsm_debug_gemm_plan writes it).  No DSM_* variable is read, nothing differs in
 * any launch of an engine on which this is never called, and the engine steps afterwards as before.  Returns 0 or <0. */
typedef struct dsm_debug_rowmap {
  int64_t bstride;
  int32_t rpb, ld, toff, pad_;
} dsm_debug_rowmap;
typedef struct dsm_debug_gemm_args {
  int32_t M, N, K;
  int32_t weight_bf16, epi, act, may_defer, norm_rms;
  int32_t knobs[5];
  int32_t w_changed; /* out */
  const float* X;
  uint64_t x_len;
  dsm_debug_rowmap xmap;
  const float* W;
  const float *bias, *scale; /* [N] or null */
  const float* res;
  uint64_t res_len;
  dsm_debug_rowmap rmap;
  float* Y; /* in: what the buffer holds before, out: after */
  uint64_t y_len;
  dsm_debug_rowmap ymap;
  float* Y2;
  uint64_t y2_len;
  dsm_debug_rowmap y2map;
  const float *norm_w, *norm_b; /* [N] */
  float* norm_out;              /* in / out, norm_len floats, rows of N from element 0 */
  uint64_t norm_len;
  float *x_back, *res_back;
} dsm_debug_gemm_args;
int dsm_debug_gemm(dsm_engine*, dsm_debug_gemm_args* args, char* plan, size_t plan_cap);

/* ------------------------------------------------------------------------------------------------
 * Audio ingest helpers (host only; SURVEY.md §8(f) rank 3, first part).
 * dsm_wav_decode: channel 0 of a RIFF/WAVE body as f32 — what srv/utils.rs:263-305 `pcm_decode` hands the worker
 * (srv/batched_asr.rs:834-842) for such a body.  *pcm_out is malloc'd; release it with dsm_free.
 * dsm_linear_resampler_*: the clients' default resampler, client/rust/kyutai-client-core/src/audio.rs:133-183
 * (`LinearResampler::process_into`), streaming.  The Opus codec is the host's callback; the Ogg container and mp3 are built (below).
 * ------------------------------------------------------------------------------------------------ */
int dsm_wav_decode(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out);

/* r04 — the rest of srv/utils.rs:263-305 `pcm_decode` for the bodies the reference's own samples use (audio/bria.mp3 of
 * BASELINE.json configs[0], loona.mp3, sample_fr_hibiki_*.mp3) and srv/batched_asr.rs:834-842 `kaudio::resample(&pcm, rate, 24000)`:
 *   dsm_mp3_decode   MPEG-1 Audio Layer III (ISO/IEC 11172-3; mono, stereo, joint stereo; bit reservoir; ID3v2 / Xing / ID3v1
 *                    skipped as symphonia's reader does), channel 0 as f32 in [-1, 1], no gapless trimming (FormatOptions::default()).
 *                    symphonia is an un-vendored crate and no decoder is importable offline: PARITY UNPINNED against it; the
 *                    tables and the filter bank are pinned by their defining properties (tests/test_mp3.py).  MPEG-2 / 2.5 and
 *                    Layers I / II: DSM_ERR_IO.
 *   dsm_mp3_probe    the frame walk alone (headers + side information): counts, bit rate, sync losses.
 *   dsm_resample     whole-buffer polyphase windowed-sinc resampler for a rational ratio (Kaiser, 32 zero crossings, cut-off
 *                    0.95 of the lower Nyquist) in the place of kaudio::resample (un-vendored; parity unpinned).
 *   dsm_pcm_decode   RIFF/WAVE or mp3 by magic — the call the worker front end makes on a request body.
 * Outputs are malloc'd (dsm_free). */
typedef struct dsm_mp3_info {
  int sample_rate, channels, bitrate_kbps /* first frame */, vbr;
  int frames;       /* audio frames (1152 samples each); a leading Xing / Info / VBRI frame is metadata and not counted */
  int info_frames, resyncs, huffman_overruns, frames_without_reservoir;
  uint64_t id3v2_bytes, junk_bytes; /* junk: bytes skipped between frames after the first one (sync losses) */
} dsm_mp3_info;
int dsm_mp3_decode(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out);
int dsm_mp3_decode_info(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, dsm_mp3_info* info);
int dsm_mp3_probe(const uint8_t* bytes, size_t len, dsm_mp3_info* out);
int dsm_resample(const float* in, size_t n, int rate_in, int rate_out, float** out, size_t* n_out);
int dsm_pcm_decode(const uint8_t* bytes, size_t len, float** pcm_out, size_t* n_out, int* sample_rate_out);
/* test aids (tests/test_mp3.py): the synthesis bank, the Huffman tables and the IMDCT on their own */
int dsm_mp3_test_synth(const float* subbands, int slots, float* pcm);
int dsm_mp3_test_tables(int table, int* xlen, int* linbits, uint16_t* codes, uint8_t* lens, int cap);
int dsm_mp3_test_imdct(const float* spectrum, int block_type, float* out);
void dsm_free(void*);
/* Ogg container demultiplexer (RFC 3533 pages -> RFC 7845 Opus packets) for InMsg::OggOpus bodies, the container half of
 * kaudio::ogg_opus::Decoder (srv/batched_asr.rs:894,941-949): streaming (bytes may be split anywhere), CRC-checked,
 * resynchronises after damage, drops packets whose beginning or middle was lost.  No Opus codec is built here: the
 * packets go to the decoder the host already has (dsm_worker_set_opus_decoder, or the caller's own loop). */
typedef struct dsm_ogg_demux dsm_ogg_demux;
dsm_ogg_demux* dsm_ogg_demux_new(void);
void dsm_ogg_demux_free(dsm_ogg_demux*);
int dsm_ogg_demux_push(dsm_ogg_demux*, const uint8_t* bytes, size_t len); /* -> packets waiting, or <0 */
int dsm_ogg_demux_next(dsm_ogg_demux*, const uint8_t** packet, size_t* len, int* is_header); /* 1 / 0; pointer valid until the next call */
int dsm_ogg_demux_info(const dsm_ogg_demux*, int* channels, int* pre_skip, uint32_t* input_rate, uint64_t* pages_ok, uint64_t* pages_bad);
/* Ogg multiplexer: the container half of kaudio::ogg_opus::Encoder on the TTS output side (srv/tts.rs:75-76,188-260):
 * dsm_ogg_mux_header = `header_data()` (OpusHead page + OpusTags page), dsm_ogg_mux_page = the page `encode_page(pcm)`
 * emits for one 80 ms frame, from the Opus packets of the host's encoder.  Both return the page bytes' count and write
 * them when they fit in cap (a page that does not fit is not consumed: call again with a larger buffer). */
typedef struct dsm_ogg_mux dsm_ogg_mux;
dsm_ogg_mux* dsm_ogg_mux_new(uint32_t serial, int channels, uint32_t input_sample_rate, int pre_skip);
void dsm_ogg_mux_free(dsm_ogg_mux*);
int dsm_ogg_mux_header(dsm_ogg_mux*, uint8_t* out, size_t cap);
int dsm_ogg_mux_page(dsm_ogg_mux*, const uint8_t* const* packets, const size_t* lens, int n_packets, uint64_t samples_48k,
                     int end_of_stream, uint8_t* out, size_t cap);
typedef struct dsm_resampler dsm_resampler;
dsm_resampler* dsm_linear_resampler_new(uint32_t in_rate_hz, uint32_t out_rate_hz);
size_t dsm_linear_resampler_process(dsm_resampler*, const float* in, size_t n_in, float* out, size_t out_cap);
void dsm_linear_resampler_free(dsm_resampler*);

/* ------------------------------------------------------------------------------------------------
 * Host worker above the engine: moshi-server's BatchedAsr module minus the sockets.
 * Wire format: rmp_serde "struct map" encoding of the internally tagged enums InMsg / OutMsg (srv/asr.rs:15-34):
 * a msgpack map whose first entry is "type": <variant>, followed by the variant's fields in declaration order;
 * usize / i64 in their smallest msgpack integer form, f64 as 0xcb, f32 as 0xca (srv/batched_asr.rs:877-880,969-975;
 * client/rust/kyutai-client/src/stt/protocol.rs:47-62, whose test vector at :82-97 pins the encoding).
 * ------------------------------------------------------------------------------------------------ */
enum { DSM_IN_INIT = 0, DSM_IN_MARKER = 1, DSM_IN_AUDIO = 2, DSM_IN_OGGOPUS = 3, DSM_IN_PING = 4 };
typedef struct dsm_in_msg {
  int kind;
  int64_t id;          /* Marker */
  const float* pcm;    /* Audio */
  size_t n_pcm;
  const uint8_t* data; /* OggOpus */
  size_t n_data;
} dsm_in_msg;
enum { DSM_OUT_WORD = 0, DSM_OUT_ENDWORD = 1, DSM_OUT_MARKER = 2, DSM_OUT_STEP = 3, DSM_OUT_ERROR = 4, DSM_OUT_READY = 5 };
typedef struct dsm_out_msg {
  int kind;
  const char* text;      /* Word.text / Error.message (UTF-8, NUL terminated) */
  double time;           /* Word.start_time / EndWord.stop_time */
  int64_t id;            /* Marker */
  uint64_t step_idx;     /* Step */
  const float* prs;
  size_t n_prs;
  uint64_t buffered_pcm;
} dsm_out_msg;
/* Encoders return the encoded size (and write it when it fits in cap); decoders return 0 or DSM_ERR_IO. */
int dsm_inmsg_encode(const dsm_in_msg*, uint8_t* buf, size_t cap);   /* client: protocol.rs encode_in_msg */
int dsm_outmsg_encode(const dsm_out_msg*, uint8_t* buf, size_t cap); /* server: send_loop serialisation */
int dsm_inmsg_decode(const uint8_t* bytes, size_t len, dsm_in_msg* out, float* pcm_buf, size_t pcm_cap,
                     uint8_t* data_buf, size_t data_cap);            /* server: rmp_serde::from_slice::<InMsg> */
int dsm_outmsg_decode(const uint8_t* bytes, size_t len, dsm_out_msg* out, char* text_buf, size_t text_cap,
                      float* prs_buf, size_t prs_cap);               /* client: protocol.rs decode_out_msg */

/* ---- SentencePiece, native (csrc/dsm_spm.h; host only, no device work) ----
 * The reference's servers hold a sentencepiece::SentencePieceProcessor: `text_tokenizer.encode(word)` in the TTS recv_loop
 * (srv/tts.rs:485) and `decode_piece_ids` for every Word (srv/batched_asr.rs:667, srv/tts.rs:598).  These calls are that
 * object for UNIGRAM models: the model file's normalizer (precompiled charsmap, whitespace rules, dummy prefix), the best
 * unigram path with the module's own tie-breaks, byte fallback, and DecodeIds.  The model file is untrusted input: every
 * length in it is checked and nothing of it is executed.
 *   dsm_spm_load / dsm_spm_load_bytes   DSM_ERR_IO: unreadable, truncated or malformed.  DSM_ERR_INVALID: a well-formed model
 *     outside the subset — BPE, WORD or CHAR model type, USER_DEFINED pieces, treat_whitespace_as_suffix, a denormalizer
 *     charsmap (DESIGN.md says why).  dsm_spm_last_error(NULL) is the calling thread's message.
 *   dsm_spm_special_ids   unk = the piece of type UNKNOWN; bos / eos / pad = trainer_spec's ids, -1 where that id is not a
 *     CONTROL piece of the model (SentencePieceProcessor::bos_id() and friends answer the same).  Any pointer may be NULL.
 *   dsm_spm_encode   SentencePieceProcessor::Encode(text) -> ids.  Returns the count; when it exceeds `cap` nothing is
 *     written and the count says what is needed.  Malformed UTF-8 encodes as U+FFFD per byte, like the module.
 *   dsm_spm_decode   DecodeIds: returns the byte length of the UTF-8 text (no NUL is written), same convention.  An id >=
 *     dsm_spm_vocab_size is DSM_ERR_INVALID (dsm_spm_last_error(tok): the calling thread's message), not a skip.
 * A loaded tokenizer is immutable: any number of threads may use it at once. */
typedef struct dsm_spm dsm_spm;
int dsm_spm_load(const char* path, dsm_spm** out);
int dsm_spm_load_bytes(const uint8_t* bytes, size_t len, dsm_spm** out);
void dsm_spm_free(dsm_spm*);
const char* dsm_spm_last_error(const dsm_spm*);
int dsm_spm_vocab_size(const dsm_spm*);
int dsm_spm_special_ids(const dsm_spm*, int* unk, int* bos, int* eos, int* pad);
int64_t dsm_spm_encode(const dsm_spm*, const char* utf8, size_t len, uint32_t* ids_out, size_t cap);
int64_t dsm_spm_decode(const dsm_spm*, const uint32_t* ids, size_t n, char* out, size_t cap);

/* text_tokenizer.decode_piece_ids (srv/batched_asr.rs:667): write the UTF-8 text of the pieces, return its length or <0.
 * The override of dsm_worker_set_tokenizer_file; with neither, a Word carries the decimal piece ids separated by spaces. */
typedef int (*dsm_detok_fn)(void* user, const uint32_t* tokens, int n_tokens, char* out, size_t cap);

typedef struct dsm_worker dsm_worker;
int dsm_worker_create(dsm_engine*, dsm_worker** out);  /* slot table of batch_size channels (srv/batched_asr.rs:762-790) */
/* The four moshi-core calls the worker makes (encode_step :362, reset_batch_idx :468, step_tokens :476 + its
 * Vec<AsrMsg>), as a table, so that the worker logic can be driven by something other than the HIP engine (the
 * test-suite plugs the CPU oracle in here; the product path is dsm_worker_create). */
typedef struct dsm_worker_backend {
  void* self;
  int batch_size, asr_delay_in_tokens, extra_heads_num;
  int (*encode_step)(void* self, const float* pcm /*[B*1920]*/, const uint8_t* mask /*[B]*/); /* codes stay inside */
  int (*reset_slot)(void* self, int slot);
  int (*step_tokens)(void* self, const uint8_t* mask, uint32_t* text_tokens_out /*[B]*/, float* prs_out /*[heads*B]*/);
  int (*poll_msgs)(void* self, dsm_asr_msg* msgs, int cap, uint32_t* tokens_out, int tokens_cap);
  const char* (*last_error)(void* self); /* may be NULL */
  /* optional pair (both or neither): the run-ahead forms — encode returns at once with a ticket naming the frame's codes,
   * the model side consumes tickets in order (dsm_mimi_encode_step_async / dsm_asr_step_tokens_ticket).  With them the
   * worker lets dsm_worker_step_encode run up to three frames ahead of dsm_worker_step_model; without them one. */
  int (*encode_async)(void* self, const float* pcm, const uint8_t* mask, int* ticket);
  int (*step_ticket)(void* self, int ticket, const uint8_t* mask, uint32_t* text_tokens_out, float* prs_out);
  int text_out_vocab_size; /* the LM's text vocabulary, 0 = not known: dsm_worker_set_tokenizer_file checks against it */
} dsm_worker_backend;
int dsm_worker_create_with_backend(const dsm_worker_backend*, dsm_worker** out);
void dsm_worker_destroy(dsm_worker*);
const char* dsm_worker_last_error(const dsm_worker*);
void dsm_worker_set_detokenizer(dsm_worker*, dsm_detok_fn, void* user);
/* Word.text = the native decode of the word's tokens with this SentencePiece model (dsm_spm_decode).  A dsm_detok_fn, if set,
 * still wins; with neither the decimal ids stay.  A token outside the model (the `?` of srv/batched_asr.rs:667, where the
 * reference's loop ends) makes that step return DSM_ERR_STATE with the message.  DSM_ERR_IO / DSM_ERR_INVALID as
 * dsm_spm_load; DSM_ERR_INVALID also when the model has more pieces than the backend's text_out_vocab_size (an engine-backed
 * worker knows its own).  The previous tokenizer, if any, stays on failure. */
int dsm_worker_set_tokenizer_file(dsm_worker*, const char* path);
/* on != 0: every Word message becomes a map of type, text, start_time, logprob and min_logprob — the mean and the minimum (f64)
 * of the word's token log-probabilities (dsm_asr_poll_word_scores); both keys are left out of a Word one of whose tokens has no
 * recorded score.  Turns the engine's token scores on (top_n 0) if they are off.  Off, the default, keeps the reference's wire
 * bytes; decoders that ignore unknown map keys (serde's default, dsm_outmsg_decode) read either form.  DSM_ERR_STATE on a worker
 * with a caller-supplied backend (dsm_worker_create_with_backend), which has no scores. */
int dsm_worker_set_word_scores(dsm_worker*, int on);
/* BatchedAsr::channels (:796-808) + the Init that handle_socket / handle_query send (:833,893).  Returns the slot
 * (batch_idx) or DSM_ERR_STATE when no slot is free ("Server at capacity - no free channels available", :875). */
int dsm_worker_open(dsm_worker*, uint64_t* channel_id);
int dsm_worker_close(dsm_worker*, int slot);           /* the socket went away: the slot is recycled by the next step */
/* One binary websocket message from the client (recv_loop, :927-951): 0 queued, 1 undecodable and skipped (malformed,
 * larger than 64 MiB, or nested deeper than rmp_serde's limit of 1024: the reference logs and carries on),
 * DSM_ERR_STATE closed channel / OggOpus (no Opus decoder in this build). */
int dsm_worker_send(dsm_worker*, int slot, const uint8_t* msgpack, size_t len);
/* handle_query (srv/batched_asr.rs:811-851): a whole audio FILE (RIFF/WAVE or MPEG-1 Layer III) as the request on a freshly opened channel
 * (dsm_worker_open queued the Init) — queues the decoded clip resampled to 24 kHz, Marker { id: 0 } and ten seconds of silence; the transcript is complete when the Marker returns. */
int dsm_worker_send_body(dsm_worker*, int slot, const uint8_t* body, size_t len);
/* One pass of encoder_loop -> model_loop -> post_process (:314-522) on the calling thread: 1 a step ran, 0 idle, <0 engine error. */
int dsm_worker_step(dsm_worker*);
/* The same work as the reference's threads split it (:314 encoder_loop, :432 model_loop + :414 post_process), for a host
 * that runs them on two threads: dsm_worker_step_encode cuts the next frame from the sockets' queues, starts its Mimi encode and
 * queues a PipelineMsg (1 produced, 0 idle or queue full); dsm_worker_step_model takes the oldest one through slot resets,
 * step_tokens and the message fan-out (1 ran, 0 nothing queued).  With the engine as backend the encode of frame n+1 overlaps
 * the LM step of frame n on the GPU; every client receives the same messages in the same order as with dsm_worker_step. */
int dsm_worker_step_encode(dsm_worker*);
int dsm_worker_step_model(dsm_worker*);
/* Next serialised OutMsg for the slot's socket (send_loop, :960-985): 1 written, 0 none; *len = its size. */
int dsm_worker_recv(dsm_worker*, int slot, uint8_t* buf, size_t cap, size_t* len);
int dsm_worker_buffered(dsm_worker*, int slot);        /* samples waiting in the channel's queue (Step.buffered_pcm) */
/* The codec half of kaudio::ogg_opus::Decoder::new(24000, FRAME_SIZE) (srv/batched_asr.rs:894): decode ONE Opus packet of
 * the slot's stream to 24 kHz mono f32 (libopus on the host side: opus_decode_float at 24 kHz), return the sample count or
 * <0.  With a decoder set, InMsg::OggOpus bodies are demultiplexed per channel (dsm_ogg_demux) and every audio packet is
 * decoded and queued like InMsg::Audio (:941-947); a decode error is reported and skipped like the reference logs it.
 * Without one, dsm_worker_send keeps refusing OggOpus messages (DSM_ERR_STATE). */
typedef int (*dsm_opus_decode_fn)(void* user, int slot, const uint8_t* packet, size_t len, float* pcm_out, size_t cap);
/* Threading contract of the decoder callback: it is called from the thread that called dsm_worker_send, OUTSIDE
 * the worker lock and under the CHANNEL's own lock only — concurrently for different slots, never concurrently for one slot;
 * `slot` tells the callback which per-socket decoder state to use.  It must not call back into dsm_worker_* for the same slot. */
void dsm_worker_set_opus_decoder(dsm_worker*, dsm_opus_decode_fn, void* user);

/* ---- text bias: per-stream keyword boosting and token bias (this project's own; the reference takes the arg-max or the Gumbel
 * sample of the raw row and stops, core/asr.rs:208-216).  Off by default: a step then enqueues exactly what it enqueues without
 * this section.  Definition (csrc/dsm_text_bias.h, bit-identical on host and device): a BIAS SET holds token biases — (token,
 * bias), bias finite or -inf (a ban) — and keywords, each ONE word as its piece ids with a boost > 0 in logit units, compiled
 * into a trie.  A slot carries the set it is attached to (0 = none) and a trie node (0 the root, DSM_BIAS_DEAD outside the trie
 * or where the engine cannot know the position).  The step's pick runs on x = raw logits + token biases + the boosts of the
 * node's edges (two f32 adds in that order), then the node advances: token 0 or 3 -> root, else along the token, else DEAD.
 * The raw logits are not modified: "lm.logits", the token scores and the extra heads see what they see without this section.
 * Greedy shallow fusion: a partial match that then fails is not taken back; multi-word phrases are out of scope.
 *   dsm_asr_set_text_bias   engine-wide switch; on: lm_pick_biased_kernel picks every slot's token (one launch in place of the
 *     arg-max / Gumbel launch, none added).  Any time between steps; waits for calls in progress on other threads; a change makes
 *     the LM step's graphs settle again (two eager steps).  DSM_ERR_INVALID when text_out_vocab_size is above 15360 (the row is
 *     staged in LDS) or below 4.  Turning it off keeps sets and attachments; turning it on puts every attached slot's node at
 *     the root (never stepped) or DEAD.
 *   dsm_asr_bias_create     compiles and uploads a set (one device allocation); *set_out is a positive handle, never reused in
 *     the engine's life.  DSM_ERR_INVALID — engine unchanged — for more than DSM_BIAS_MAX_TOKENS token biases, a token >=
 *     text_out_vocab_size or listed twice, a bias that is +inf or NaN, a keyword of 0 or more than DSM_BIAS_MAX_KEYWORD_TOKENS
 *     pieces, a piece >= text_out_vocab_size or equal to 0 / 3, a boost that is not finite and > 0, more than DSM_BIAS_MAX_NODES
 *     trie nodes; DSM_ERR_STATE when DSM_BIAS_MAX_SETS - 1 sets exist.
 *   dsm_asr_bias_create_text  the same with the keywords as UTF-8 words: each is encoded alone with dsm_spm_encode.  A word is
 *     refused by index in dsm_last_error when it contains whitespace, encodes to nothing or to more than 32 pieces, or yields a
 *     piece >= text_out_vocab_size or equal to 0 / 3.  (The pieces a checkpoint emits for a word may differ from the tokenizer's
 *     best segmentation: DESIGN.md.)
 *   dsm_asr_bias_destroy    DSM_ERR_STATE ("in use by n slots") while attached; dsm_destroy frees what is left.
 *   dsm_asr_bias_info       nodes, edges, token biases, current references, device bytes; any pointer may be NULL.
 *   dsm_asr_set_bias        attaches `slot` to `set` (0 detaches), whether the switch is on or off.  Synchronises the engine's
 *     streams.  The node becomes the root if the slot has not stepped since its last reset (host step index 0), else DEAD, which
 *     heals at the stream's next 0 / 3.  dsm_asr_reset_slot keeps the attachment and returns the node to the root.  Slot
 *     snapshots do not carry either: after dsm_asr_import_slots / dsm_asr_move_slots the destination keeps ITS OWN attachment and
 *     its node is DEAD, or the root when the imported item's step index is 0; the blob's bytes do not depend on this section.
 *   dsm_asr_bias_state      the slot's set and node as of the last finished step (synchronises).  Without a set the node reads DEAD.
 *   dsm_text_bias_compile   host only, no device: the flat table of a set.  *needed (optional) receives its length in words;
 *     words_out NULL: size query only; cap < needed: DSM_ERR_INVALID.  dsm_last_error(NULL) is the calling thread's message.
 *   dsm_text_bias_pick_host host only: the definition for one row — token and next node.  table NULL (table_words 0): no set,
 *     the node comes back unchanged.  The table is checked in full first; DSM_ERR_INVALID for a malformed one, a table that names
 *     a token >= V, a node that is neither DEAD nor below its node count, temperature > 0 with a NULL key or a position that is
 *     not a multiple of 16.
 *   dsm_debug_text_pick     test aid: runs the step's KERNEL on caller rows — host logits [n][V], nodes_in [n], for temperature > 0
 *     rng_keys [n][8] and rng_pos [n]; tokens_out [n], nodes_out [n].  `set` 0: no set.  4 <= V <= 15360 and above every token
 *     of the set.  Synchronises the model stream.
 *   dsm_worker_set_bias     dsm_asr_set_bias for an open channel's slot; the worker detaches the slot when the channel closes
 *     (in the dsm_worker_step_encode that recycles the slot; frames of it still in the run-ahead pipeline then step detached)
 *     and, for channels still open, in dsm_worker_destroy — which therefore comes before dsm_destroy of the engine.
 *     DSM_ERR_STATE for a closed channel or a worker built with dsm_worker_create_with_backend.  The wire format does not change. */
#define DSM_BIAS_MAX_TOKENS 1024
#define DSM_BIAS_MAX_KEYWORD_TOKENS 32
#define DSM_BIAS_MAX_NODES 65535
#define DSM_BIAS_MAX_SETS 256
#define DSM_BIAS_DEAD 0xFFFFFFFFu
typedef struct { uint32_t token; float bias; } dsm_bias_token;
typedef struct { const uint32_t* tokens; int n_tokens; float boost; } dsm_bias_keyword;
int dsm_asr_set_text_bias(dsm_engine*, int on);
int dsm_asr_bias_create(dsm_engine*, const dsm_bias_token*, int n_tokens, const dsm_bias_keyword*, int n_keywords, int* set_out);
int dsm_asr_bias_create_text(dsm_engine*, const dsm_spm*, const char* const* words, const float* boosts, int n_words,
                             const dsm_bias_token*, int n_tokens, int* set_out);
int dsm_asr_bias_destroy(dsm_engine*, int set);
int dsm_asr_bias_info(dsm_engine*, int set, int* nodes, int* edges, int* tokens, int* refs, size_t* device_bytes);
int dsm_asr_set_bias(dsm_engine*, int slot, int set /* 0 detaches */);
int dsm_asr_bias_state(dsm_engine*, int slot, int* set, uint32_t* node);
int dsm_text_bias_compile(const dsm_bias_token* tokens, int n_tokens, const dsm_bias_keyword* keywords, int n_keywords, int V,
                          uint32_t* words_out, size_t cap, size_t* needed);
int dsm_text_bias_pick_host(const uint32_t* table, size_t table_words, uint32_t node, const float* logits, int V, float temperature,
                            const uint32_t* rng_key /*8 words or NULL*/, uint64_t rng_pos, uint32_t* token, uint32_t* node_out);
int dsm_debug_text_pick(dsm_engine*, int set, const float* logits, int n, int V, const uint32_t* nodes_in, float temperature,
                        const uint32_t* rng_keys /*[n][8] or NULL*/, const uint64_t* rng_pos, uint32_t* tokens_out, uint32_t* nodes_out);
int dsm_worker_set_bias(dsm_worker*, int slot, int set);

/* ---- ingest: per-stream input sample rate and sample format, resampled on the device (this project's own: the reference
 * resamples request bodies only, srv/batched_asr.rs:835-838, and its sockets must send 24 kHz f32).  Off by default: nothing is
 * allocated and every other call enqueues exactly what it enqueues without this section.  Definition (csrc/dsm_pcm_format.h,
 * bit-identical on host and device): a slot's FORMAT is a sample rate — 8000 .. 48000 Hz with a whole number F_in = 2 rate / 25
 * of samples per 80 ms frame (8000, 11025, 16000, 22050, 32000, 44100, 48000 among them) — and a sample format: DSM_PCM_F32,
 * DSM_PCM_S16 (little endian, v / 32768), DSM_PCM_MULAW, DSM_PCM_ALAW (ITU-T G.711, expanded to 16 bits, then as s16).  With x
 * the slot's decoded input since the format was set and y = dsm_resample(x, rate, 24000), step t hands Mimi
 * z_t[n] = y[1920 t + n - D], 0 in front of the stream: D = floor(half L / M) output samples (102 at 8 kHz, 51 at 16 kHz, 33 at
 * 44.1 kHz, 34 at 48 kHz; 0 at 24 kHz) is the format's latency.  24000 / F32 is the pass-through format and every slot's default.
 *   dsm_asr_set_ingest        engine-wide switch.  On: allocates the section (per-slot format and history, the raw staging at the
 *     largest pitch, 15360 bytes a slot) and lets the raw calls run; off: they return DSM_ERR_STATE.  The plain calls are the
 *     same either way.  Formats and histories stay across off / on.
 *   dsm_asr_set_input_format  sets the slot's format and clears its history on both Mimi sides (the next frame is the first of
 *     a stream).  Between steps; synchronises the engine's streams.  DSM_ERR_INVALID, nothing changed, for a rate or format
 *     outside the definition; DSM_ERR_STATE while ingest is off.  dsm_mimi_reset_slot clears the encoder side's history,
 *     dsm_asr_reset_slot the model side's; the format stays across resets, as a bias attachment does.
 *   dsm_asr_input_format      the slot's format, its frame in samples and bytes, and D; any pointer may be NULL.
 *   dsm_mimi_encode_step_raw, _raw_async, _raw_dev, dsm_asr_step_raw  their plain siblings — same streams, events, ticket ring and
 *     lock — with "upload 1920 floats per slot" replaced by "upload the raw rows, launch ingest_resample_kernel", which writes
 *     the frames where the upload writes them.  raw: [B][pitch_bytes], slot b's frame in the first frame_bytes(b) bytes of its
 *     row; pitch_bytes % 16 == 0, at most 15360, and at least every ACTIVE slot's frame_bytes (DSM_ERR_INVALID otherwise, no
 *     state changed; the _dev variant, whose mask is on the device, checks against every slot).  A masked-off slot's row is not
 *     read and its history stays.  d_raw must be 16-byte aligned.
 *   dsm_debug_ingest_read     test aid: the frames [B][1920] the side's (0 encoder, 1 model) last raw call handed to Mimi.
 *   dsm_ingest_host_*         host only, no device: one slot's streaming state going through the same header functions as the
 *     kernel.  dsm_ingest_host takes one frame of the format's frame_bytes and writes 1920 samples.
 *   dsm_ingest_describe       host only: the twelve words of a format's descriptor (rate, fmt, L, M, half, taps, F_in,
 *     frame_bytes, D, 0, table words, 0), or DSM_ERR_INVALID with dsm_last_error(NULL) saying why.
 *   dsm_ingest_g711_table     host only: the 256 expanded 16-bit values of DSM_PCM_MULAW / DSM_PCM_ALAW.
 *   dsm_worker_set_input_rate  for an open channel of an engine-backed worker (DSM_ERR_STATE on a caller-supplied backend or
 *     a closed channel, and once the channel's audio has been cut into frames; DSM_ERR_INVALID for a rate outside the
 *     definition): the channel's InMsg::Audio samples are f32 at `hz`.  Turns ingest on if it is off.  The channel's queue is cut
 *     into frames of F_in samples; Step.buffered_pcm counts the channel's own samples; a Marker counts queued frames in units of
 *     F_in and is due ONE STEP LATER than on a 24 kHz channel, because the last D output samples in front of it land in the next
 *     frame.  While any open channel has such a rate, dsm_worker_step and dsm_worker_step_encode call
 *     dsm_mimi_encode_step_raw_async (every channel's frame in a row of the longest open frame); when none has, exactly what they
 *     call without this section.  The rate returns to 24000 when the channel goes back to the free list and in
 *     dsm_worker_destroy, where and as the bias detach.  Wire bytes are unchanged.  dsm_worker_send_body and the Opus callback
 *     path stay as they are (24 kHz).
 * Slot snapshots carry neither format nor history: after dsm_asr_import_slots / dsm_asr_move_slots the destination slot keeps
 * ITS OWN; the caller sets the format after an import (which also clears the history).  Sample formats other than f32 are an
 * engine-level feature, for hosts that own their sockets. */
#define DSM_PCM_F32 0
#define DSM_PCM_S16 1
#define DSM_PCM_MULAW 2
#define DSM_PCM_ALAW 3
typedef struct dsm_ingest_host_state dsm_ingest_host_state;
int dsm_asr_set_ingest(dsm_engine*, int on);
int dsm_asr_set_input_format(dsm_engine*, int slot, int sample_rate_hz, int sample_format);
int dsm_asr_input_format(dsm_engine*, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples_24k);
int dsm_mimi_encode_step_raw(dsm_engine*, const void* raw, size_t pitch_bytes, const uint8_t* mask, uint32_t* codes_out, int* produced);
int dsm_mimi_encode_step_raw_async(dsm_engine*, const void* raw, size_t pitch_bytes, const uint8_t* mask, int* ticket);
int dsm_mimi_encode_step_raw_dev(dsm_engine*, const void* d_raw, size_t pitch_bytes, const uint8_t* d_mask, uint32_t* d_codes_out);
int dsm_asr_step_raw(dsm_engine*, const void* raw, size_t pitch_bytes, const uint8_t* mask, uint32_t* codes_out,
                     uint32_t* text_tokens_out, float* vad_prs_out);
int dsm_debug_ingest_read(dsm_engine*, int side, float* out /*[B][1920]*/);
dsm_ingest_host_state* dsm_ingest_host_new(int sample_rate_hz, int sample_format);
void dsm_ingest_host_free(dsm_ingest_host_state*);
int dsm_ingest_host(dsm_ingest_host_state*, const void* raw_frame, float* out1920);
int dsm_ingest_describe(int sample_rate_hz, int sample_format, uint32_t* words12);
int dsm_ingest_g711_table(int sample_format, int16_t* out256);
int dsm_worker_set_input_rate(dsm_worker*, int slot, int hz);

/* ---- clips: a slot's audio known beforehand, resident on the device in its own ingest format, K steps per visit (this project's
 * own shape of the reference's request path, BatchedAsr::handle_query, srv/batched_asr.rs:810-854: decode, queue the audio, then
 * silence, cut the queue into whole frames, collect Word / EndWord; the STT sibling of dsm_tts_run / dsm_tts_collect).  Off by
 * default: nothing is allocated and every other call enqueues exactly what it enqueues without this section.  Definition
 * (csrc/dsm_asr_clip.h, host only; the device side copies the bytes it names): a slot's CLIP is clip_bytes bytes in the slot's
 * ingest format; FRAME i is bytes [i frame_bytes, (i + 1) frame_bytes) of the clip followed by endless silence — the byte 0x00
 * for DSM_PCM_F32 and DSM_PCM_S16, 0xFF for DSM_PCM_MULAW (expands to 0), 0xD5 for DSM_PCM_ALAW (the idle code, expands to +8) —
 * so a clip need not end on a frame or a sample.  With n_audio = ceil(clip_bytes / frame_bytes), a CLOSED slot takes frames
 * 0 .. n_audio + flush_frames - 1, one per step, and is then DONE; an OPEN slot takes a frame only once all of its bytes were
 * pushed, else it sits the step out (mask 0) and is WAITING.  The frames go through ingest_resample_kernel, the encoder-side
 * Mimi and the LM exactly as through dsm_mimi_encode_step_raw_async + dsm_asr_step_tokens_ticket with the same rows and
 * masks: codes, tokens, VAD values, scores, messages, HostItem and model_step_idx end bit for bit the same.
 *   dsm_asr_set_clips     engine-wide switch, between steps.  On: turns ingest on if it is off and allocates [B][max] device
 *     bytes for the clips (max_clip_bytes_per_slot, 1 .. 2^31, rounded up to 16), a pinned mirror of them that pushes append to,
 *     the block's table and its records for DSM_ASR_RUN_MAX steps.  A second call with another size: DSM_ERR_STATE.  Off: the
 *     calls below return DSM_ERR_STATE; DSM_ERR_STATE while a slot has a clip or a block waits.
 *   dsm_asr_clip_begin    dsm_asr_reset_slot, dsm_mimi_reset_slot and dsm_asr_set_input_format(rate, fmt) for the slot, then the
 *     slot has an empty open clip and is RUNNING.  flush_frames: silent frames behind the audio (the reference appends
 *     asr_delay_in_tokens + a margin of frames of zeros behind a body).  DSM_ERR_STATE, nothing touched: the slot has a clip
 *     already (dsm_asr_reset_slot ends one), a block waits, an encode ticket is outstanding.  DSM_ERR_INVALID: a rate or format
 *     outside the ingest definition, flush_frames < 0.
 *   dsm_asr_clip_push     appends n bytes (any count: a push need not end on a frame or a sample).  The copy rides the encoder
 *     stream out of the pinned mirror, so the caller's buffer is free on return.  DSM_ERR_STATE, nothing changed: beyond
 *     max_clip_bytes_per_slot, a closed slot, a slot without a clip, a block waits.
 *   dsm_asr_clip_close    no more bytes: the clip's last, partial frame and the flush follow.  Closing twice is fine.
 *   dsm_asr_run           n_steps (1 .. DSM_ASR_RUN_MAX) steps of every slot with a clip; enqueue only: no synchronise, no
 *     download.  The host knows every slot's frame index and mask for all the steps (the schedule depends on no data) and
 *     uploads them as one table; per step the encoder stream cuts the frames (asr_clip_frame_kernel), resamples and encodes,
 *     the model stream takes codes AND mask in one hand-off and steps the LM into the engine's own buffers, and every stream
 *     group records its slots' results behind its step.  Slots without a clip, WAITING and DONE slots are masked off.  The
 *     captured graphs are the per-step calls' (no new variants, nothing settles again).  DSM_ERR_STATE, nothing touched: a
 *     block waits for dsm_asr_collect, n_steps out of range, an encode ticket is outstanding.  While a block waits, the
 *     stepping calls (dsm_mimi_encode_step*, dsm_asr_step_*), dsm_asr_reset_slot, dsm_mimi_reset_slot and
 *     dsm_asr_set_input_format return DSM_ERR_STATE; between blocks the per-step calls serve the other slots (mask[b] = 1 on a
 *     slot with a clip: DSM_ERR_STATE, nothing changed; the _dev calls, whose mask is on the device, are the caller's to keep
 *     off clip slots).
 *   dsm_asr_collect       the one synchronise of a block; fills the caller's arrays (any may be NULL) for the n_steps of the
 *     block: stepped [n][B] (the slot took a frame in that step), text_token [n][B] and vad_prs [n][heads][B] (defined where
 *     stepped is 1), logprob [n][B] (NaN while token scores are off), status [B] (DSM_ASR_CLIP_* after the block), and the
 *     messages of every step — assemble_words replayed once per step over the records, so dsm_asr_poll_msgs afterwards holds the
 *     last step's — with msg_step[i] = the index in the block of the step that msgs[i] belongs to, their tokens in msg_tokens
 *     and the tokens' log-probabilities in msg_logprobs (tokens_offset counts from the block's first token).  n_msgs / n_tokens
 *     are what the block produced; entries beyond msgs_cap / tokens_cap are dropped.  DSM_ERR_STATE when no block waits.
 *   dsm_asr_clip_status   DSM_ASR_CLIP_* of the slot: as of the last dsm_asr_run, push or close.  dsm_asr_reset_slot ends a clip
 *     (-> IDLE); its bytes are dropped.
 *   dsm_asr_clip_frame_host  host only: frame `frame_index` of a clip in (rate, fmt) -> frame_out (the format's frame_bytes
 *     bytes); returns frame_bytes, or DSM_ERR_INVALID with dsm_last_error(NULL) saying why.  clip may be NULL for 0 bytes.
 *   dsm_asr_clip_host_*   host only, no device: the schedule dsm_asr_run goes through, for B slots with a cap per clip — begin
 *     (frame_bytes from (rate, fmt)), push (a byte count), close, reset, status, and run: n_steps rows of frame [n][B] and
 *     mask [n][B] (DSM_ERR_INVALID for n_steps outside 1 .. DSM_ASR_RUN_MAX).  Refusals as the engine's.
 * Slot snapshots carry no clip: dsm_asr_export_slots / dsm_asr_move_slots of a slot with a clip return DSM_ERR_STATE.  The worker
 * does not use this section: dsm_worker_send_body stays as it is. */
#define DSM_ASR_RUN_MAX 16 /* steps per block: one row of the table and of the records each */
enum { DSM_ASR_CLIP_IDLE = 0, DSM_ASR_CLIP_RUNNING = 1, DSM_ASR_CLIP_WAITING = 2, DSM_ASR_CLIP_DONE = 3 };
typedef struct dsm_asr_block {
  int n_steps;              /* out: steps in the block */
  uint8_t* stepped;         /* [n][B] */
  uint32_t* text_token;     /* [n][B] */
  float* vad_prs;           /* [n][extra_heads_num][B] */
  float* logprob;           /* [n][B] */
  dsm_asr_msg* msgs;        /* [msgs_cap] */
  int* msg_step;            /* [msgs_cap] */
  int msgs_cap;
  int n_msgs;               /* out */
  uint32_t* msg_tokens;     /* [tokens_cap] */
  float* msg_logprobs;      /* [tokens_cap] */
  int tokens_cap;
  int n_tokens;             /* out */
  int* status;              /* [B] DSM_ASR_CLIP_* after the block */
} dsm_asr_block;
typedef struct dsm_asr_clip_host_state dsm_asr_clip_host_state;
int dsm_asr_set_clips(dsm_engine*, int on, size_t max_clip_bytes_per_slot);
int dsm_asr_clip_begin(dsm_engine*, int slot, int sample_rate_hz, int sample_format, int flush_frames);
int dsm_asr_clip_push(dsm_engine*, int slot, const void* bytes, size_t n);
int dsm_asr_clip_close(dsm_engine*, int slot);
int dsm_asr_run(dsm_engine*, int n_steps);
int dsm_asr_collect(dsm_engine*, dsm_asr_block* out);
int dsm_asr_clip_status(dsm_engine*, int slot);
int dsm_asr_clip_frame_host(const void* clip, size_t clip_bytes, int sample_rate_hz, int sample_format, uint64_t frame_index,
                            void* frame_out);
dsm_asr_clip_host_state* dsm_asr_clip_host_new(int batch_size, size_t max_clip_bytes_per_slot);
void dsm_asr_clip_host_free(dsm_asr_clip_host_state*);
int dsm_asr_clip_host_begin(dsm_asr_clip_host_state*, int slot, int sample_rate_hz, int sample_format, int flush_frames);
int dsm_asr_clip_host_push(dsm_asr_clip_host_state*, int slot, size_t n);
int dsm_asr_clip_host_close(dsm_asr_clip_host_state*, int slot);
int dsm_asr_clip_host_reset(dsm_asr_clip_host_state*, int slot);
int dsm_asr_clip_host_status(dsm_asr_clip_host_state*, int slot);
int dsm_asr_clip_host_run(dsm_asr_clip_host_state*, int n_steps, uint32_t* frame /*[n][B]*/, uint8_t* mask /*[n][B]*/);

/* ---- egress: per-slot TTS output sample rate and sample format, resampled and encoded on the device (this project's own: the
 * reference's TTS sockets send 24 kHz f32, srv/tts.rs:528-544).  The ingest section run the other way — the same rates, the same
 * DSM_PCM_* formats, the same filter family.  Off by default: nothing is allocated and every other call enqueues exactly what it
 * enqueues without this section.  Definition (csrc/dsm_pcm_format.h, bit-identical on host and device): a slot's FORMAT is a sample
 * rate — 8000 .. 48000 Hz with a whole number F_out = 2 rate / 25 of samples per 80 ms frame — and a sample format:
 * DSM_PCM_F32, DSM_PCM_S16 (little endian, rint(v 32768) clamped, NaN 0), DSM_PCM_MULAW, DSM_PCM_ALAW (ITU-T G.711 of that
 * 16-bit value).  With x the slot's emitted PCM since the format was set (only the frames whose valid flag is 1) and
 * y = dsm_resample(x, 24000, rate), the slot's e-th emitted frame is z_e[n] = y[F_out e + n - D], 0 in front of the stream:
 * D = floor(half L / M) output samples (34 at 8 kHz, 33 at 11.025 kHz, 34 at 16 kHz, 33 at 22.05 kHz, 45 at 32 kHz, 62 at
 * 44.1 kHz, 68 at 48 kHz; 0 at 24 kHz) is the format's latency.  The last D output samples of a generation (at most 4.25 ms)
 * are never delivered; there is no flush.  24000 / F32 is the pass-through format and every slot's default: the step's 1920
 * floats bit for bit.
 *   dsm_tts_set_egress        engine-wide switch; needs an attached Mimi, no deferred step waiting and no block waiting
 *     (DSM_ERR_STATE otherwise, nothing changed).  On: allocates the section (per-slot format and history, the coefficient
 *     arena, a device staging of 15360 bytes a slot, a pinned raw buffer beside every queue entry), lets the raw calls run, and
 *     every decode then downloads the raw rows IN THE PLACE of the 1920 floats; dsm_tts_step_pcm, dsm_tts_recv_pcm and
 *     dsm_tts_collect with out->pcm on a decode block return DSM_ERR_STATE with nothing touched.  Off: the raw calls return
 *     DSM_ERR_STATE.  Formats and histories stay across off / on.
 *   dsm_tts_set_output_format sets the slot's format and clears its history (the next emitted frame is the first of a stream).
 *     Between steps; synchronises the engine's streams.  DSM_ERR_INVALID, nothing changed, for a rate or format outside the
 *     definition; DSM_ERR_STATE while egress is off or a block waits.  dsm_tts_reset_slot clears the history and keeps the
 *     format; frames queued before a reset are still delivered.
 *   dsm_tts_output_format     the slot's format, its frame in samples and bytes, and D; any pointer may be NULL.
 *   dsm_tts_step_raw, dsm_tts_recv_raw, dsm_tts_collect_raw  their plain siblings dsm_tts_step_pcm, dsm_tts_recv_pcm and
 *     dsm_tts_collect — same streams, events, queue of two, lock, emit rule and refusals.  raw: [B][pitch_bytes] (collect:
 *     [n][B][pitch_bytes]); slot b's frame is the first frame_bytes(b) bytes of its row, the rest of the row and the row of a
 *     slot that did not emit are not written.  pitch_bytes % 16 == 0, at most 15360, and at least every active slot's
 *     frame_bytes (DSM_ERR_INVALID otherwise, no state changed; recv and collect check the slots that emitted, and the entry
 *     or block stays queued).  dsm_tts_step_raw with raw_out NULL defers, as dsm_tts_step_pcm with pcm_out NULL
 *     (pitch_bytes is not read then).
 *     dsm_tts_collect_raw fills `out` exactly as dsm_tts_collect does, and out->pcm must be NULL.
 *   dsm_tts_debug_egress      test aid: with egress on and nothing queued, runs egress_resample_kernel once on the caller's
 *     frames [B][1920] and valid flags [B] through the slots' current formats and histories (which advance) and returns the rows.
 *   dsm_egress_host_*         host only, no device: one slot's streaming state going through the same header functions as the
 *     kernel.  dsm_egress_host takes one emitted frame of 1920 samples and writes the format's frame_bytes.
 *   dsm_egress_describe       host only: the twelve words of a format's descriptor (rate, fmt, L, M, half, taps, F_out,
 *     frame_bytes, D, 0, table words, 0), or DSM_ERR_INVALID with dsm_last_error(NULL) saying why.
 *   dsm_egress_encode_sample  host only: one sample through the shared encoder; writes 4, 2, 1 or 1 bytes.
 * Slot snapshots carry neither format nor history: after dsm_tts_import_slots, a move or a fork, the destination slot keeps
 * ITS OWN; the caller sets the format after an import (which also clears the history). */
typedef struct dsm_egress_host_state dsm_egress_host_state;
int dsm_tts_set_egress(dsm_tts*, int on);
int dsm_tts_set_output_format(dsm_tts*, int slot, int sample_rate_hz, int sample_format);
int dsm_tts_output_format(dsm_tts*, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples);
int dsm_tts_step_raw(dsm_tts*, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                     uint32_t* text_token_out, uint32_t* audio_out, void* raw_out /* [B][pitch_bytes] or NULL = deferred */,
                     size_t pitch_bytes, uint8_t* valid_out);
int dsm_tts_recv_raw(dsm_tts*, void* raw_out, size_t pitch_bytes, uint8_t* valid_out);
int dsm_tts_collect_raw(dsm_tts*, dsm_tts_block* out, void* raw /* [n][B][pitch_bytes] */, size_t pitch_bytes);
int dsm_tts_debug_egress(dsm_tts*, const float* pcm /*[B][1920]*/, const uint8_t* valid /*[B]*/, void* raw_out, size_t pitch_bytes);
dsm_egress_host_state* dsm_egress_host_new(int sample_rate_hz, int sample_format);
void dsm_egress_host_free(dsm_egress_host_state*);
int dsm_egress_host(dsm_egress_host_state*, const float* frame1920, void* raw_out);
int dsm_egress_describe(int sample_rate_hz, int sample_format, uint32_t* words12);
int dsm_egress_encode_sample(int sample_format, float v, void* out);

#ifdef __cplusplus
}
#endif
#endif /* DSM_H */
