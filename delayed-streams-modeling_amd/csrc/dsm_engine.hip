// dsm_engine.hip — libdsm_mi355x.so: the engine behind include/dsm.h.
//
// Host orchestration of the per-80 ms-frame batched step on one MI355X:
//   encoder side  (HIP stream "enc")   Mimi::encode_step      core/mimi.rs:195-206
//   model side    (HIP stream "model") asr::State::step_tokens core/asr.rs:147-255
// All per-slot state (conv carries, ring KV caches, ring index/position, item state) lives in
// HBM and is advanced by the kernels themselves; the only per-step host<->device traffic is the
// PCM/mask upload and the token/VAD download, like the reference (SURVEY.md §2.1 last paragraph).
// There is no CPU fallback: creation fails if no HIP device is usable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <set>
#include <vector>

#include "../../include/dsm.h"
#include "dsm_device.h"
#include "dsm_config_presets.h"
#include "dsm_gemm_plan.h"
#include "dsm_kernels.h"
#include "dsm_pcm_table.inc"
#include "dsm_numerics.h"
#include "dsm_safetensors.h"
#include "dsm_slot_blob.h"
#include "dsm_tts_slot_blob.h"
#include "dsm_tts_slot_layout.h"
#include "dsm_spm.h"
#include "dsm_slot_xfer.inc"
#include "dsm_asr_clip.h"

static thread_local std::string g_create_error;

// The library's whole environment: ten DSM_* variables (include/dsm.h lists them), read once per engine by DsmDevice::open
// after dot_mode is set.  dsm_env_int is the only getenv in csrc/; the two group counts (DSM_LM_GROUPS, DSM_TTS_GROUPS) go
// through it where they are computed.
static int dsm_env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
static void dsm_read_env(DsmDevice* e, bool stt) {
  // dot_mode 1, STT engine only: whole-K workgroups pay from 192 (n, m) tiles on (gemm_default_knobs, dsm_gemm_plan.h), and the
  // bf16 GEMMs leave the vector ALU to the attention waves, so large attention launches run three workgroups per CU (r03: 52.1 ->
  // 50.4 ms at B = 2048, 59.8 -> 56.9 at 2304; four: 53.7).  The TTS engine has always kept 384 and 60000 in both modes; the
  // difference is kept on purpose: dropping it would change which kernels a TTS step launches.
  e->chunk_loop_min_tiles = gemm_default_knobs(stt, e->dot_mode).chunk_loop_min_tiles;
  if (stt && e->dot_mode == 1) e->attn_lds_pad = 40000;
  e->use_graphs = dsm_env_int("DSM_GRAPHS", 1) != 0;
  e->fuse_qkv = dsm_env_int("DSM_FUSE_QKV", 1) != 0;
  e->stream_prio = dsm_env_int("DSM_STREAM_PRIO", 0) != 0;  // the TTS engine's two streams have no priorities: ignored there
  e->fuse_front = dsm_env_int("DSM_FUSE_FRONT", 1) != 0;
  e->chunk_loop_min_tiles = dsm_env_int("DSM_CHUNK_LOOP_MIN", e->chunk_loop_min_tiles);
  e->loop_depth = dsm_env_int("DSM_LOOP_DEPTH", e->loop_depth) == 2 ? 2 : 4;
  e->smallk_min_tiles = dsm_env_int("DSM_SMALLK_MIN", e->smallk_min_tiles);
  const int mt = dsm_env_int("DSM_SMALLK_MT", e->smallk_mt);
  if (mt == 1 || mt == 2 || mt == 4) e->smallk_mt = mt;
}


namespace {

struct Linear {  // packed weight [Npad][Kpad] (+ optional bias) on the device
  void* w = nullptr;
  float* bias = nullptr;
  int N = 0, K = 0, Npad = 0, Kpad = 0;
  bool bf16 = false;
  bool packed = false;  // bf16 only (r04): fragment-major [Npad / 16][Kpad / 32][64 lanes][8] instead of row-major (dsm_wbase)
};

struct ConvGeom {
  Linear lin;
  int in_c = 0, out_c = 0, k = 0, stride = 1;
  int S = 0;     // carried frames = k_eff - stride (dilation 1)
  int T_in = 0;  // input frames per step
  int T_out = 0;
  bool replicate = false;
};

ConvGeom over_frames(const ConvGeom& g, int r) {  // the streaming geometry of one frame, over r frames at once
  ConvGeom c = g;
  c.T_in *= r;
  c.T_out *= r;
  return c;
}

struct TLayerW {
  Linear in_proj, out_proj, ff_in, ff_out;
  float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr, *ls1 = nullptr, *ls2 = nullptr;
  // cross attention (TTS main LM, core/transformer.rs:205-330,747-763): in_proj_q, in_proj_kv, out_proj, norm_cross
  Linear ca_q, ca_kv, ca_out;
  float *ncw = nullptr, *ncb = nullptr;
};

struct TransformerW {
  dsm_transformer_config cfg{};
  int hidden = 0;
  std::vector<TLayerW> layers;
  float* inv_freq = nullptr;
  bool rope_pos_before = false;  // non-batched transformer semantics (TTS main LM)
  bool has_ca = false;           // every layer carries norm_cross + cross_attention
  int ca_norm_rms = 0;           // norm_cross: RmsNorm (eps 1e-8) instead of LayerNorm (eps 1e-5)
};

// Per-row cross-attention sources of a transformer_forward call: the projected keys / values of every batch row's ca_src
// (compute_kv, core/transformer.rs:299-318) laid out like a ring cache, [rows][H][smax][hd] per layer, so that attn_kernel
// serves them: `last` = source length - 1 plays start_pos (every one of the `len` rows is visible, no causal mask), `act`
// = the row attends this step (it is active and has a source).  `att` [rows][d] holds the attention output; rows that never
// attend keep the zeros they were created with, so their out_proj term is +0 (ca_src = None: the layer adds nothing, :753-760).
// `src` (per layer, one entry per row, device memory) says where each row's block is: its private block in k / v, or a voice
// shared with other rows (dsm_tts_voice.inc).  The attention launch reads the blocks through it, never through k / v directly.
struct CaState {
  std::vector<void*> k, v;
  std::vector<AttnRowSrc*> src;
  uint32_t* last = nullptr;
  uint8_t* act = nullptr;
  float* att = nullptr;
  int smax = 0;
};

struct TransformerState {  // per (side): ring caches + ScatteredCacheBuilder state
  std::vector<void*> k, v;  // per layer [B][H][ctx][hd]
  uint32_t *pos = nullptr, *idx = nullptr, *start_pos = nullptr, *widx = nullptr;
  float* rope_cs = nullptr;
};

struct RvqW {
  Linear input_proj, output_proj;
  int n_q = 0;
  std::vector<Linear> codebooks;  // W = embedding [bins][dim] f32, bias = c2 [bins]
};

struct MimiW {
  dsm_mimi_config cfg{};
  ConvGeom init_conv, final_conv, downsample;
  struct Stage {
    ConvGeom ra, rb, down;
  };
  std::vector<Stage> stages;
  TransformerW tr;
  RvqW rvq_first, rvq_rest;
  // decode side (core/mimi.rs:99-103, core/seanet.rs:305-468)
  struct DecStage {
    Linear up;       // convtr as a GEMM: rows kk*out_c + co, K = in_c
    float* up_bias = nullptr;
    int in_c = 0, out_c = 0, k = 0, stride = 0, T_in = 0;
    ConvGeom ra, rb;
  };
  bool has_decoder = false;
  ConvGeom dec_init, dec_final;
  std::vector<DecStage> dec_stages;
  TransformerW dec_tr;
  float* upsample_w = nullptr;  // [k][dim]
  const float** emb_ptrs = nullptr;  // device array of n_q codebook pointers
};

// The activation scratch of one transformer_forward: x (in / out), xn, q, att [rows][d] and g [rows][hidden]
struct ActScratch {
  float *x = nullptr, *xn = nullptr, *q = nullptr, *att = nullptr, *g = nullptr;
  ActScratch from_row(size_t r0, int d, int hid) const { return {x + r0 * d, xn + r0 * d, q + r0 * d, att + r0 * d, g + r0 * hid}; }
};

// The buffers of the SEANet encoder chain (alloc_seanet_enc, seanet_encode): the concat buffer in front of every convolution
// and each stage's skip input y.  The streaming encoder holds them for B slots of one frame, the clip encoder for one clip.
struct SeanetEnc {
  float* cat_init = nullptr;
  struct Stage {
    float *y = nullptr, *cat_ra = nullptr, *cat_rb = nullptr, *cat_down = nullptr;
  };
  std::vector<Stage> stages;
  float* cat_final = nullptr;
};

struct MimiState {  // one per side (encoder-thread clone / model side)
  float* pcm = nullptr;  // == enc.cat_init + S0 (the PCM frame is uploaded straight into the concat buffer)
  SeanetEnc enc;
  ActScratch act;  // the encoder transformer's
  float* cat_ds = nullptr;
  float* latent = nullptr;
  float *res_first = nullptr, *res_rest = nullptr, *pval = nullptr;
  uint32_t* pidx = nullptr;
  uint32_t* codes = nullptr;  // [B][n_q]
  TransformerState tr;
  ConvStateDesc* descs = nullptr;  // device table for the state-shift kernel
  std::vector<ConvStateDesc> h_descs;
  int ds_desc = -1;  // index of the downsample conv in descs
  bool first_call = true;
  uint8_t* mask = nullptr;  // device [B]
  // [B], in being only once slots were imported while first_call still holds (dsm_asr_import_slots): 1 = the slot carries imported
  // state, which the first call's replicate pad and zeroing must leave alone.  keep_h mirrors it on the host.
  uint8_t* keep = nullptr;
  std::vector<uint8_t> keep_h;
};

struct MimiDecState {  // Mimi::decode_step state, allocated on first use
  bool ready = false, first_call = true;
  DsmDevice::GraphSlot* graph = nullptr;  // one decode_step
  float* h_pcm_out = nullptr;             // pinned [B][DSM_FRAME_SIZE]: the host-pointer entry point's download
  uint32_t* codes = nullptr;
  uint8_t* mask = nullptr;
  // [B], TTS decode path only (dsm_tts_attach_mimi): a slot behaves as a fresh module of its own — the carry terms follow this
  // flag instead of first_call (null: module-level first call, Mimi::decode_step of one batched module)
  uint8_t* started = nullptr;
  float *q_first = nullptr, *q_rest = nullptr, *emb = nullptr, *up_carry = nullptr;
  ActScratch act;  // the decoder transformer's
  TransformerState tr;
  float* cat_init = nullptr;
  struct Stage {
    float *x = nullptr, *z = nullptr, *carry = nullptr, *y = nullptr, *cat_ra = nullptr, *cat_rb = nullptr;
  };
  std::vector<Stage> stages;
  float* cat_final = nullptr;
  float* pcm = nullptr;
  ConvStateDesc* descs = nullptr;
  std::vector<ConvStateDesc> h_descs;
};

struct LmW {
  uint16_t* text_emb = nullptr;
  uint16_t* audio_emb = nullptr;
  TransformerW tr;
  float* out_norm = nullptr;
  Linear text_linear, extra_heads;
};

struct LmState {
  ActScratch act;
  float *hidden = nullptr, *logits = nullptr, *eh = nullptr, *prs = nullptr;
  uint32_t *next_cb = nullptr, *text_token = nullptr, *text_out = nullptr, *codes_in = nullptr;
  uint8_t *first_step = nullptr, *mask = nullptr;
  uint32_t* rng_key = nullptr;             // [B][8] ChaCha12 key per slot (temperature > 0: lm_gumbel_kernel; dsm_asr_set_seed)
  unsigned long long* rng_pos = nullptr;   // [B] words drawn so far (multiples of 16)
  uint8_t* gmask = nullptr;  // per-group private copy of the step's mask (groups free-run against each other)
  TransformerState tr;
  // stream groups: slots [b0, b0+nb) of group g step on their own HIP stream so that one group's HBM-bound attention
  // overlaps another's MFMA-bound GEMMs; rows are independent, so the split changes no result
  struct Group {
    int b0 = 0, nb = 0;
    TransformerState view;  // tr with every per-slot pointer advanced to b0
  };
  std::vector<Group> groups;
};

struct HostItem {  // ItemState — core/asr.rs:15-51 (word assembly stays on the host)
  size_t step_idx = 0;
  std::vector<uint32_t> word_tokens;
  std::vector<float> word_logprobs;  // one per word token (dsm_asr_set_token_scores); NaN = not recorded (scores off, or an imported word)
  bool unended_word = false;
  double last_stop_time = 0.0;
};

}  // namespace

// The STT product on its device context: configuration, Mimi (weights, the two encoder states, the decode state), the LM,
// pinned staging, word assembly, metrics and the encoder -> model pipeline.  Device memory, pinned memory, events and graph
// slots come from DsmDevice and are released by its destructor.
struct dsm_engine : DsmDevice {
  dsm_asr_config cfg{};
  int B = 0;
  hipEvent_t ev_grp_in[kMaxGroups] = {}, ev_stagger[kMaxGroups] = {};
  bool grp_busy = false;
  bool serialize_groups = false;  // dsm_debug_serialize_groups: every group on the model stream (profiling aid)
  hipEvent_t ev_codes_consumed = nullptr;
  bool codes_consumed_valid = false;
  hipEvent_t ev_join = nullptr, ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr;
  MimiW mimi_w;
  MimiState mimi[2];
  // mimi[1] — the Mimi clone of asr::State (core/asr.rs:58), used only by dsm_asr_step_pcm[_dev] — is allocated on first use
  // (r04): a server drives the encoder-thread clone (mimi[0]) and step_tokens, and at the capacity batch the second state set is
  // 11 GB of HBM that 256 more streams' ring caches fit into
  std::atomic<bool> mimi1_ready{false};
  std::mutex mimi1_mu;
  MimiDecState dec;
  LmW lm_w;
  LmState lm;
  GraphSlot *g_enc[2] = {}, *g_grp[kMaxGroups] = {};  // one Mimi encode per side, one LM step per stream group
  // host staging (pinned)
  float* h_pcm = nullptr;
  float* h_pcm1 = nullptr;
  uint8_t* h_mask = nullptr;
  uint32_t *h_codes = nullptr, *h_text = nullptr;
  float* h_prs = nullptr;
  // host item state + message queue
  std::vector<HostItem> items;
  size_t model_step_idx = 0;
  std::vector<dsm_asr_msg> msgs;
  std::vector<uint32_t> msg_tokens;
  std::vector<float> msg_logprobs;  // moves in step with msg_tokens (dsm_asr_poll_word_scores)
  // token scores (dsm_asr_set_token_scores; dsm_token_scores.h): -1 off, else the top_n of lm_token_scores_kernel, which then
  // runs behind each group's argmax.  Device buffers [B], [B][DSM_SCORES_MAX_TOP] x 2 and their pinned mirrors, allocated by the
  // first call that turns scores on; scores_host_steps counts the host-pointer steps since the setting last changed.
  int scores_top_n = -1;
  float *scores_lp = nullptr, *scores_top_lp = nullptr, *h_scores_lp = nullptr, *h_scores_top_lp = nullptr;
  uint32_t *scores_top_id = nullptr, *h_scores_top_id = nullptr;
  size_t scores_host_steps = 0;
  // text bias (dsm_asr_set_text_bias; dsm_text_bias.h): the switch, and what lm_pick_biased_kernel reads — the descriptor table
  // [DSM_BIAS_MAX_SETS] (entry 0 = no set), each slot's descriptor index [B] and trie node [B] — allocated by the first call of
  // the section.  Host side: the sets by handle (positive, never reused), each with its table's host copy and its reference
  // count, and the handle each slot is attached to.
  struct BiasSet {
    int index = 0;  // its entry of bias_sets_d
    std::vector<uint32_t> words;
    uint32_t* d_table = nullptr;
    int refs = 0;
  };
  bool bias_on = false;
  BiasSetDesc* bias_sets_d = nullptr;
  uint32_t *bias_slot_set = nullptr, *bias_slot_node = nullptr;
  std::map<int, BiasSet> bias_sets;
  std::vector<int> bias_slot_handle;  // [B], 0 = none
  int bias_next_handle = 1;
  std::mutex bias_mu;  // the host side of the section (the worker's threads both reach it)
  // ingest (dsm_asr_set_ingest; dsm_pcm_format.h): the switch, and what ingest_resample_kernel reads — the slots' formats
  // (PcmFormatTable, dsm_pcm_table.inc: descriptors, coefficient arena, each slot's descriptor index, with their host mirrors),
  // the G.711 tables; per Mimi side the history [B][136], the "started" words [B] and the device copy of the raw rows
  // [B][15360].  Pinned: one raw staging per side and per ticket.  All of it allocated by the first dsm_asr_set_ingest(1),
  // after which ingest_fmt.ready holds.
  bool ingest_on = false;
  PcmFormatTable ingest_fmt{DSM_PCM_IN};
  float* ingest_g711_d = nullptr;
  float* ingest_hist[2] = {};
  uint32_t* ingest_started[2] = {};
  uint8_t *ingest_raw_d[2] = {}, *ingest_raw_h[2] = {}, *ingest_pipe_raw_h[4] = {};
  std::mutex ingest_mu;  // the table's host mirrors (the worker's threads both reach them)
  // clips (dsm_asr_set_clips; dsm_asr_clip.h, dsm_asr_clip.inc): the switch; the slots' clips [B][clip_cap] on the device and
  // the pinned mirror pushes append to; the schedule's slots; a block's table (per slot AsrClipSlot, then frame [K][B] and mask
  // [K][B]) on the device and pinned, its records [K][B (2 + heads)] likewise, and the steps of the block that waits for
  // dsm_asr_collect (0: none).  All of it allocated by the first dsm_asr_set_clips(1).  clip_mu: the host side of the section.
  std::atomic<bool> clips_on{false};
  size_t clip_cap = 0;
  uint8_t *clip_d = nullptr, *clip_h = nullptr;
  std::vector<dsm_asr_clip::Slot> clip_slots;
  uint8_t *clip_tab_d = nullptr, *clip_tab_h = nullptr;
  uint32_t *clip_rec_d = nullptr, *clip_rec_h = nullptr;
  int clip_blk_pending = 0;
  std::mutex clip_mu;
  // What the per-step calls and the slot resets ask first.  mask: the call's host mask, or null (a device mask, a reset).
  // Nothing to ask while the section is off.
  int clip_guard(const uint8_t* mask) {
    if (!clips_on.load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::mutex> lk(clip_mu);
    if (clip_blk_pending) { set_error("a block of %d steps waits for dsm_asr_collect", clip_blk_pending); return DSM_ERR_STATE; }
    for (int b = 0; mask && b < B; ++b)
      if (mask[b] && clip_slots[(size_t)b].status != DSM_ASR_CLIP_IDLE) {
        set_error("slot %d has a clip: dsm_asr_run steps it (dsm_asr_reset_slot ends the clip)", b);
        return DSM_ERR_STATE;
      }
    return 0;
  }
  // the same for the calls that name slots (snapshots carry no clip; a format belongs to its clip): none of them has a clip
  int clip_guard_slots(const int* slots, int n, const char* who) {
    if (!clips_on.load(std::memory_order_acquire)) return 0;
    if (int rc = clip_guard(nullptr)) return rc;
    std::lock_guard<std::mutex> lk(clip_mu);
    for (int i = 0; i < n; ++i)
      if (slots[i] >= 0 && slots[i] < B && clip_slots[(size_t)slots[i]].status != DSM_ASR_CLIP_IDLE) {
        set_error("%s: slot %d has a clip (dsm_asr_reset_slot ends it)", who, slots[i]);
        return DSM_ERR_STATE;
      }
    return 0;
  }
  dsm_metrics metrics{};
  // run-ahead pipeline between the encoder thread and the model thread (dsm_mimi_encode_step_async /
  // dsm_asr_step_tokens_ticket): the reference's sync_channel(100) of PipelineMsg (srv/batched_asr.rs:291), here a ring of
  // kPipe frames: pinned staging for the PCM + mask, a private device copy of the frame's codes, one event "encoded" and
  // one "consumed" per entry.
  static constexpr int kPipe = 4;
  struct PipeSlot {
    float* h_pcm = nullptr;
    uint8_t* h_mask = nullptr;
    uint32_t* d_codes = nullptr;
    hipEvent_t ev_done = nullptr, ev_consumed = nullptr;
    bool in_flight = false;  // encoded (or being encoded) and not yet handed to the model side
  };
  PipeSlot pipe[kPipe];
  int pipe_next = 0;
  bool pipe_ready = false;
  std::mutex pipe_mu;
  // slot snapshots (dsm_asr_export_slots / import / move; dsm_slot_state.inc): the section table of a slot's state — LM, then
  // mimi[0], then as the optional group mimi[1] — and the staging buffers (dsm_slot_xfer.inc).  Built by the first call that needs it.
  SlotXfer xfer;
  struct {  // sections the importer range-checks
    int lm_idx = -1, text_token = -1, first_step = -1, rng_pos = -1, next_cb = -1, mimi_idx = -1;
  } xsec;
};

// ----------------------------------------------------------------------------------------------
// weight loading
// ----------------------------------------------------------------------------------------------
namespace {

struct Loader {
  DsmDevice* e;
  dsm_st_file* f;
  bool failed = false;
  std::vector<float> get(int64_t numel, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
    char name[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    std::vector<float> out((size_t)numel);
    if (failed || e->skip_host_weights()) return out;  // measure / attach: sizes only, nothing is read
    char err[512];
    if (dsm_st_read_f32(f, name, numel, out.data(), err, sizeof err)) {
      e->set_error("%s", err);
      failed = true;
    }
    return out;
  }
  bool has(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    char name[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    if (e->wmode == DsmDevice::W_ATTACH) {  // no checkpoint on this rank: replay the loading rank's answers, in order
      if (e->manifest_pos >= e->manifest.size()) { failed = true; e->set_error("weight manifest exhausted"); return false; }
      return e->manifest[e->manifest_pos++] != 0;
    }
    const bool found = dsm_st_find(f, name) != nullptr;
    if (e->wmode == DsmDevice::W_LOAD) e->manifest.push_back(found ? 1 : 0);
    return found;
  }
};

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// pack [N][K] f32 row-major into the GEMM layout [Npad][Kpad] (zero padded)
// bf16 weights (the LM's) are stored FRAGMENT-MAJOR since r04: the 16 rows x 32 k block that one wave loads as its MFMA A operand
// (lane (r, q) = 8 consecutive k of row r) is 1 KB contiguous, tile (n / 16, k / 32) at ((n / 16) * (Kpad / 32) + k / 32) * 512
// elements, lane q * 16 + r inside it — every weight load instruction covers eight full 128-byte lines instead of sixteen half
// lines 4 KB apart, and a wave's chunk is 8 KB of one DRAM page run (experiments/gemm_wk_probe: QKV / gate launches -10 %).
// split_row: a row offset the kernels address as a tile origin (the gate's up half at +hidden): must be a multiple of 16, else
// the matrix stays row-major.  The layout depends on the configuration alone, so every rank that attaches to an arena agrees on it.
int pack_linear(DsmDevice* e, Linear* L, const float* w, int N, int K, bool bf16, const float* bias, int split_row = 0) {
  L->packed = bf16 && (split_row % 16 == 0);
  L->N = N;
  L->K = K;
  L->Npad = round_up(N, 64) + 64;  // the tiled kernel reads whole 64-row tiles (and the gate's up-tile at +hidden)
  L->Kpad = round_up(K, 32);
  L->bf16 = bf16;
  size_t n = (size_t)L->Npad * L->Kpad;
  const bool skip = e->skip_host_weights();
  if (bf16) {
    std::vector<uint16_t> p(skip ? 0 : n, 0);
    if (!skip) {
      const size_t nblk = (size_t)L->Kpad >> 5;
      for (int i = 0; i < N; ++i)
        for (int j = 0; j < K; ++j) {
          const size_t at = L->packed ? ((((size_t)i >> 4) * nblk + ((size_t)j >> 5)) * 64 + (size_t)(((j >> 3) & 3) * 16 + (i & 15))) * 8 + (j & 7)
                                      : (size_t)i * L->Kpad + j;
          p[at] = dsm_f32_to_bf16(w[(size_t)i * K + j]);
        }
    }
    uint16_t* d = nullptr;
    if (int rc = e->upload_w(&d, p.data(), n)) return rc;
    L->w = d;
  } else {
    std::vector<float> p(skip ? 0 : n, 0.0f);
    if (!skip)
      for (int i = 0; i < N; ++i) memcpy(&p[(size_t)i * L->Kpad], &w[(size_t)i * K], sizeof(float) * K);
    float* d = nullptr;
    if (int rc = e->upload_w(&d, p.data(), n)) return rc;
    L->w = d;
  }
  if (bias) {
    std::vector<float> pb((size_t)L->Npad, 0.0f);
    memcpy(pb.data(), bias, sizeof(float) * N);
    if (int rc = e->upload_w(&L->bias, pb.data(), pb.size())) return rc;
  }
  return 0;
}

// conv1d_weight_norm — core/conv.rs:27-45
std::vector<float> load_conv_weight(Loader& ld, const char* prefix, int out_c, int in_c, int k) {
  if (ld.has("%s.weight", prefix)) return ld.get((int64_t)out_c * in_c * k, "%s.weight", prefix);
  std::vector<float> g = ld.get(out_c, "%s.weight_g", prefix);
  std::vector<float> v = ld.get((int64_t)out_c * in_c * k, "%s.weight_v", prefix);
  for (int o = 0; o < out_c; ++o) {
    float ss = 0.0f;
    for (int i = 0; i < in_c * k; ++i) ss = ss + v[(size_t)o * in_c * k + i] * v[(size_t)o * in_c * k + i];
    float nrm = sqrtf(ss);
    for (int i = 0; i < in_c * k; ++i) v[(size_t)o * in_c * k + i] = v[(size_t)o * in_c * k + i] * g[o] / nrm;
  }
  return v;
}

int load_conv(DsmDevice* e, Loader& ld, ConvGeom* c, const char* prefix, int in_c, int out_c, int k, int stride,
              bool bias, bool replicate, const char* wkey = nullptr) {
  char p[256];
  if (wkey)
    snprintf(p, sizeof p, "%s", wkey);
  else
    snprintf(p, sizeof p, "%s.conv.conv", prefix);
  std::vector<float> w = load_conv_weight(ld, p, out_c, in_c, k);
  std::vector<float> b;
  if (bias) b = ld.get(out_c, "%s.bias", p);
  if (ld.failed) return DSM_ERR_IO;
  // [out_c][in_c][k] -> [out_c][k*in_c] (kk-major reduction index)
  std::vector<float> r((size_t)out_c * k * in_c);
  for (int o = 0; o < out_c; ++o)
    for (int ci = 0; ci < in_c; ++ci)
      for (int kk = 0; kk < k; ++kk) r[((size_t)o * k + kk) * in_c + ci] = w[((size_t)o * in_c + ci) * k + kk];
  c->in_c = in_c;
  c->out_c = out_c;
  c->k = k;
  c->stride = stride;
  c->S = k - stride;
  c->replicate = replicate;
  return pack_linear(e, &c->lin, r.data(), out_c, k * in_c, false, bias ? b.data() : nullptr);
}

int gating_hidden(const dsm_transformer_config& c) {  // core/batched_transformer.rs:153-157
  return c.dim_feedforward == 4 * c.d_model ? 11 * c.d_model / 4 : 2 * c.dim_feedforward / 3;
}

int load_transformer(DsmDevice* e, Loader& ld, TransformerW* t, const dsm_transformer_config& cfg,
                     const char* prefix, bool bf16) {
  t->cfg = cfg;
  const int d = cfg.d_model, hd = d / cfg.num_heads;
  t->hidden = cfg.gating ? gating_hidden(cfg) : cfg.dim_feedforward;
  t->layers.resize(cfg.num_layers);
  std::vector<float> inv(hd / 2);
  for (int i = 0; i < hd / 2; ++i)  // RotaryEmbedding::new — core/transformer.rs:386-392
    inv[i] = (float)(1.0 / pow((double)cfg.max_period, (double)(2 * i) / (double)hd));
  if (int rc = e->upload_w(&t->inv_freq, inv.data(), inv.size())) return rc;
  for (int l = 0; l < cfg.num_layers; ++l) {
    TLayerW& L = t->layers[l];
    {
      auto w = ld.get((int64_t)3 * d * d, "%s.layers.%d.self_attn.in_proj_weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.in_proj, w.data(), 3 * d, d, bf16, nullptr)) return rc;
    }
    {
      auto w = ld.get((int64_t)d * d, "%s.layers.%d.self_attn.out_proj.weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.out_proj, w.data(), d, d, bf16, nullptr)) return rc;
    }
    for (int which = 1; which <= 2; ++which) {
      float** w = which == 1 ? &L.n1w : &L.n2w;
      float** b = which == 1 ? &L.n1b : &L.n2b;
      std::vector<float> wv, bv;
      if (cfg.norm == 1) {
        wv = ld.get(d, "%s.layers.%d.norm%d.alpha", prefix, l, which);
      } else {
        bv = ld.get(d, "%s.layers.%d.norm%d.bias", prefix, l, which);
        if (ld.has("%s.layers.%d.norm%d.alpha", prefix, l, which))
          wv = ld.get(d, "%s.layers.%d.norm%d.alpha", prefix, l, which);
        else
          wv = ld.get(d, "%s.layers.%d.norm%d.weight", prefix, l, which);
      }
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = e->upload_w(w, wv.data(), wv.size())) return rc;
      if (!bv.empty())
        if (int rc = e->upload_w(b, bv.data(), bv.size())) return rc;
    }
    if (cfg.gating) {
      auto wi = ld.get((int64_t)2 * t->hidden * d, "%s.layers.%d.gating.linear_in.weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.ff_in, wi.data(), 2 * t->hidden, d, bf16, nullptr, t->hidden)) return rc;
      auto wo = ld.get((int64_t)d * t->hidden, "%s.layers.%d.gating.linear_out.weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.ff_out, wo.data(), d, t->hidden, bf16, nullptr)) return rc;
    } else {
      auto wi = ld.get((int64_t)t->hidden * d, "%s.layers.%d.linear1.weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.ff_in, wi.data(), t->hidden, d, bf16, nullptr)) return rc;
      auto wo = ld.get((int64_t)d * t->hidden, "%s.layers.%d.linear2.weight", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = pack_linear(e, &L.ff_out, wo.data(), d, t->hidden, bf16, nullptr)) return rc;
    }
    if (cfg.layer_scale) {
      auto s1 = ld.get(d, "%s.layers.%d.layer_scale_1.scale", prefix, l);
      auto s2 = ld.get(d, "%s.layers.%d.layer_scale_2.scale", prefix, l);
      if (ld.failed) return DSM_ERR_IO;
      if (int rc = e->upload_w(&L.ls1, s1.data(), s1.size())) return rc;
      if (int rc = e->upload_w(&L.ls2, s2.data(), s2.size())) return rc;
    }
  }
  return 0;
}

int check_transformer_config(DsmDevice* e, const dsm_transformer_config& t) {
  if (t.d_model % t.num_heads || t.d_model % 32 || t.d_model > 4096) {
    e->set_error("d_model must be a multiple of num_heads and of 32, and <= 4096 (the row-norm kernels keep a row in registers)");
    return DSM_ERR_INVALID;
  }
  const int hd = t.d_model / t.num_heads;
  if (hd != 32 && hd != 64 && hd != 128) { e->set_error("head_dim %d unsupported (32, 64, 128)", hd); return DSM_ERR_INVALID; }
  return 0;
}

// The LM trunk both engines share (srv/batched_asr.rs:738-745, srv/tts.rs:345): bf16 text and audio embedding tables, the
// transformer, out_norm, text_linear — in this order, which is the STT weight arena's carve order.  Cfg: dsm_asr_config or
// dsm_tts_config (same field names).
template <typename Cfg>
int load_lm_trunk(DsmDevice* e, Loader& ld, LmW* w, const Cfg& c) {
  const int d = c.lm.d_model;
  const bool skip = e->skip_host_weights();
  auto te = ld.get((int64_t)c.text_in_vocab_size * d, "text_emb.weight");
  if (ld.failed) return DSM_ERR_IO;
  std::vector<uint16_t> tb(skip ? 0 : te.size());
  for (size_t i = 0; i < tb.size(); ++i) tb[i] = dsm_f32_to_bf16(te[i]);
  if (int rc = e->upload_w(&w->text_emb, tb.data(), te.size())) return rc;
  const size_t per = (size_t)c.audio_vocab_size * d;
  std::vector<uint16_t> ab(skip ? 0 : (size_t)c.audio_codebooks * per);
  for (int i = 0; i < c.audio_codebooks && !ld.failed && !skip; ++i) {
    auto ae = ld.get((int64_t)per, "emb.%d.weight", i);
    for (size_t j = 0; j < ae.size(); ++j) ab[(size_t)i * per + j] = dsm_f32_to_bf16(ae[j]);
  }
  if (ld.failed) return DSM_ERR_IO;
  if (int rc = e->upload_w(&w->audio_emb, ab.data(), (size_t)c.audio_codebooks * per)) return rc;
  if (int rc = load_transformer(e, ld, &w->tr, c.lm, "transformer", true)) return rc;
  auto on = ld.get(d, "out_norm.alpha");
  auto tl = ld.get((int64_t)c.text_out_vocab_size * d, "text_linear.weight");
  if (ld.failed) return DSM_ERR_IO;
  if (int rc = e->upload_w(&w->out_norm, on.data(), on.size())) return rc;
  return pack_linear(e, &w->text_linear, tl.data(), c.text_out_vocab_size, d, true, nullptr);
}

int alloc_transformer_state(DsmDevice* e, TransformerState* st, const dsm_transformer_config& cfg, int B, int T,
                            bool kv_bf16) {
  const int H = cfg.num_heads, hd = cfg.d_model / H;
  size_t per = (size_t)B * H * cfg.context * hd;
  st->k.resize(cfg.num_layers);
  st->v.resize(cfg.num_layers);
  for (int l = 0; l < cfg.num_layers; ++l) {
    if (kv_bf16) {
      uint16_t *k = nullptr, *v = nullptr;
      if (int rc = e->dalloc(&k, per)) return rc;
      if (int rc = e->dalloc(&v, per)) return rc;
      st->k[l] = k;
      st->v[l] = v;
    } else {
      float *k = nullptr, *v = nullptr;
      if (int rc = e->dalloc(&k, per)) return rc;
      if (int rc = e->dalloc(&v, per)) return rc;
      st->k[l] = k;
      st->v[l] = v;
    }
  }
  if (int rc = e->dalloc(&st->pos, B)) return rc;
  if (int rc = e->dalloc(&st->idx, B)) return rc;
  if (int rc = e->dalloc(&st->start_pos, B)) return rc;
  if (int rc = e->dalloc(&st->widx, (size_t)B * T)) return rc;
  if (int rc = e->dalloc(&st->rope_cs, (size_t)B * T * hd)) return rc;
  return 0;
}

int alloc_act(DsmDevice* e, ActScratch* a, size_t rows, int d, int hid) {
  for (float** p : {&a->x, &a->xn, &a->q, &a->att})
    if (int rc = e->dalloc(p, rows * d)) return rc;
  return e->dalloc(&a->g, rows * hid);
}

// A stream group's view of per-row state: every per-row pointer advanced to row r0 (T = 1).
void offset_rings(std::vector<void*>& k, std::vector<void*>& v, size_t bytes) {
  for (size_t l = 0; l < k.size(); ++l) {
    k[l] = (char*)k[l] + bytes;
    v[l] = (char*)v[l] + bytes;
  }
}
TransformerState group_view(const TransformerState& full, const dsm_transformer_config& tc, size_t kv_elem_bytes, int r0) {
  TransformerState v = full;
  const int hd = tc.d_model / tc.num_heads;
  offset_rings(v.k, v.v, (size_t)r0 * tc.d_model * tc.context * kv_elem_bytes);  // [rows][H][ctx][hd]
  v.pos += r0; v.idx += r0; v.start_pos += r0; v.widx += r0;
  v.rope_cs += (size_t)r0 * hd;
  return v;
}
CaState group_view(const CaState& full, int d_model, size_t kv_elem_bytes, int r0) {
  CaState v = full;
  offset_rings(v.k, v.v, (size_t)r0 * d_model * full.smax * kv_elem_bytes);  // [rows][H][smax][hd]
  for (AttnRowSrc*& s : v.src) s += r0;
  v.last += r0; v.act += r0;
  v.att += (size_t)r0 * d_model;
  return v;
}

int load_rvq(DsmDevice* e, Loader& ld, RvqW* r, const char* prefix, int n_q, const dsm_mimi_config& m) {
  const int bins = m.quantizer_bins, dim = m.quantizer_dim;
  r->n_q = n_q;
  auto ip = ld.get((int64_t)dim * m.dimension, "%s.input_proj.weight", prefix);
  if (ld.failed) return DSM_ERR_IO;
  if (int rc = pack_linear(e, &r->input_proj, ip.data(), dim, m.dimension, false, nullptr)) return rc;
  if (ld.has("%s.output_proj.weight", prefix)) {  // decode side; STT-only checkpoints may omit nothing, but be lenient
    auto op = ld.get((int64_t)m.dimension * dim, "%s.output_proj.weight", prefix);
    if (ld.failed) return DSM_ERR_IO;
    if (int rc = pack_linear(e, &r->output_proj, op.data(), m.dimension, dim, false, nullptr)) return rc;
  }
  r->codebooks.resize(n_q);
  for (int i = 0; i < n_q; ++i) {
    auto usage = ld.get(bins, "%s.vq.layers.%d._codebook.cluster_usage", prefix, i);
    auto esum = ld.get((int64_t)bins * dim, "%s.vq.layers.%d._codebook.embedding_sum", prefix, i);
    if (ld.failed) return DSM_ERR_IO;
    std::vector<float> c2(bins);
    for (int j = 0; j < bins; ++j) {  // EuclideanCodebook::new — core/quantization.rs:86-95
      float u = usage[j] > 1e-5f ? usage[j] : 1e-5f;
      float ss = 0.0f;
      for (int dd = 0; dd < dim; ++dd) {
        float v = esum[(size_t)j * dim + dd] / u;
        esum[(size_t)j * dim + dd] = v;
        ss = ss + v * v;
      }
      c2[j] = ss / 2.0f;
    }
    if (int rc = pack_linear(e, &r->codebooks[i], esum.data(), bins, dim, false, c2.data())) return rc;
  }
  return 0;
}

int load_mimi(DsmDevice* e, Loader& ld, MimiW* m, const dsm_mimi_config& cfg) {
  m->cfg = cfg;
  char p[128];
  int mult = 1, idx = 0, T = DSM_FRAME_SIZE;
  snprintf(p, sizeof p, "encoder.model.%d", idx);
  if (int rc = load_conv(e, ld, &m->init_conv, p, cfg.channels, mult * cfg.n_filters, cfg.kernel_size, 1, true, false)) return rc;
  m->init_conv.T_in = T;
  m->init_conv.T_out = T;
  idx += 1;
  m->stages.resize(cfg.n_ratios);
  for (int i = 0; i < cfg.n_ratios; ++i) {
    int ratio = cfg.ratios[cfg.n_ratios - 1 - i];  // core/seanet.rs:194 ratios.iter().rev()
    int dim = mult * cfg.n_filters, hidden = dim / cfg.compress;
    MimiW::Stage& st = m->stages[i];
    snprintf(p, sizeof p, "encoder.model.%d.block.1", idx);
    if (int rc = load_conv(e, ld, &st.ra, p, dim, hidden, cfg.residual_kernel_size, 1, true, false)) return rc;
    snprintf(p, sizeof p, "encoder.model.%d.block.3", idx);
    if (int rc = load_conv(e, ld, &st.rb, p, hidden, dim, 1, 1, true, false)) return rc;
    idx += 1;
    snprintf(p, sizeof p, "encoder.model.%d", idx + 1);
    if (int rc = load_conv(e, ld, &st.down, p, dim, dim * 2, ratio * 2, ratio, true, false)) return rc;
    idx += 2;
    st.ra.T_in = st.ra.T_out = st.rb.T_in = st.rb.T_out = st.down.T_in = T;
    if (T % ratio) {
      e->set_error("frame of %d samples does not divide by the encoder ratios", DSM_FRAME_SIZE);
      return DSM_ERR_INVALID;
    }
    T /= ratio;
    st.down.T_out = T;
    mult *= 2;
  }
  snprintf(p, sizeof p, "encoder.model.%d", idx + 1);
  if (int rc = load_conv(e, ld, &m->final_conv, p, mult * cfg.n_filters, cfg.dimension, cfg.last_kernel_size, 1, true, false)) return rc;
  m->final_conv.T_in = m->final_conv.T_out = T;
  if (int rc = load_transformer(e, ld, &m->tr, cfg.transformer, "encoder_transformer.transformer", false)) return rc;
  if (int rc = load_conv(e, ld, &m->downsample, nullptr, cfg.dimension, cfg.dimension, 2 * cfg.downsample_stride,
                         cfg.downsample_stride, false, true, "downsample.conv.conv.conv"))
    return rc;
  m->downsample.T_in = T;
  if (T % cfg.downsample_stride) {
    e->set_error("encoder frames per step (%d) do not divide by the downsample stride", T);
    return DSM_ERR_INVALID;
  }
  m->downsample.T_out = T / cfg.downsample_stride;
  if (m->downsample.T_out != 1) {
    e->set_error("expected exactly one latent frame per step, got %d", m->downsample.T_out);
    return DSM_ERR_INVALID;
  }
  if (int rc = load_rvq(e, ld, &m->rvq_first, "quantizer.rvq_first", 1, cfg)) return rc;
  if (cfg.quantizer_n_q > 1)
    if (int rc = load_rvq(e, ld, &m->rvq_rest, "quantizer.rvq_rest", cfg.quantizer_n_q - 1, cfg)) return rc;
  // ---- decode side: only if the checkpoint carries it (the STT worker never calls decode_step) ----
  m->has_decoder = ld.has("decoder.model.0.conv.conv.weight") || ld.has("decoder.model.0.conv.conv.weight_v");
  if (!m->has_decoder) return 0;
  {
    int mult = 1 << cfg.n_ratios, idx = 0, T = m->final_conv.T_out;  // frames per step at the encoder rate (2)
    char p[128];
    snprintf(p, sizeof p, "decoder.model.%d", idx);
    if (int rc = load_conv(e, ld, &m->dec_init, p, cfg.dimension, mult * cfg.n_filters, cfg.kernel_size, 1, true, false)) return rc;
    m->dec_init.T_in = m->dec_init.T_out = T;
    idx += 1;
    m->dec_stages.resize(cfg.n_ratios);
    for (int i = 0; i < cfg.n_ratios; ++i) {
      const int ratio = cfg.ratios[i];
      MimiW::DecStage& st = m->dec_stages[i];
      st.in_c = mult * cfg.n_filters;
      st.out_c = st.in_c / 2;
      st.k = 2 * ratio;
      st.stride = ratio;
      st.T_in = T;
      snprintf(p, sizeof p, "decoder.model.%d.convtr.convtr", idx + 1);
      std::vector<float> w;
      if (ld.has("%s.weight", p)) {
        w = ld.get((int64_t)st.in_c * st.out_c * st.k, "%s.weight", p);
      } else {  // weight norm over dims (1,2) of [in_c, out_c, k] — core/conv.rs:136-139
        auto g = ld.get(st.in_c, "%s.weight_g", p);
        w = ld.get((int64_t)st.in_c * st.out_c * st.k, "%s.weight_v", p);
        for (int ci = 0; ci < st.in_c && !ld.failed; ++ci) {
          float ss = 0.0f;
          const size_t n = (size_t)st.out_c * st.k;
          for (size_t j = 0; j < n; ++j) ss = ss + w[ci * n + j] * w[ci * n + j];
          float nrm = sqrtf(ss);
          for (size_t j = 0; j < n; ++j) w[ci * n + j] = w[ci * n + j] * g[ci] / nrm;
        }
      }
      auto b = ld.get(st.out_c, "%s.bias", p);
      if (ld.failed) return DSM_ERR_IO;
      // [in_c][out_c][k] -> rows (kk*out_c + co), K = in_c
      std::vector<float> r((size_t)st.k * st.out_c * st.in_c);
      for (int ci = 0; ci < st.in_c; ++ci)
        for (int co = 0; co < st.out_c; ++co)
          for (int kk = 0; kk < st.k; ++kk)
            r[((size_t)kk * st.out_c + co) * st.in_c + ci] = w[((size_t)ci * st.out_c + co) * st.k + kk];
      if (int rc = pack_linear(e, &st.up, r.data(), st.k * st.out_c, st.in_c, false, nullptr)) return rc;
      if (int rc = e->upload_w(&st.up_bias, b.data(), b.size())) return rc;
      idx += 2;
      T *= ratio;
      const int dim = st.out_c, hidden = dim / cfg.compress;
      snprintf(p, sizeof p, "decoder.model.%d.block.1", idx);
      if (int rc = load_conv(e, ld, &st.ra, p, dim, hidden, cfg.residual_kernel_size, 1, true, false)) return rc;
      snprintf(p, sizeof p, "decoder.model.%d.block.3", idx);
      if (int rc = load_conv(e, ld, &st.rb, p, hidden, dim, 1, 1, true, false)) return rc;
      st.ra.T_in = st.ra.T_out = st.rb.T_in = st.rb.T_out = T;
      idx += 1;
      mult /= 2;
    }
    snprintf(p, sizeof p, "decoder.model.%d", idx + 1);
    if (int rc = load_conv(e, ld, &m->dec_final, p, cfg.n_filters, cfg.channels, cfg.last_kernel_size, 1, true, false)) return rc;
    m->dec_final.T_in = m->dec_final.T_out = T;
    if (T != DSM_FRAME_SIZE) {
      e->set_error("decoder emits %d samples per step, expected %d", T, DSM_FRAME_SIZE);
      return DSM_ERR_INVALID;
    }
    if (int rc = load_transformer(e, ld, &m->dec_tr, cfg.transformer, "decoder_transformer.transformer", false)) return rc;
    const int st_ = cfg.downsample_stride, dim = cfg.dimension;
    auto uw = ld.get((int64_t)dim * 2 * st_, "upsample.convtr.convtr.convtr.weight");  // [dim][1][k]
    if (ld.failed) return DSM_ERR_IO;
    std::vector<float> ur((size_t)2 * st_ * dim);
    for (int c = 0; c < dim; ++c)
      for (int kk = 0; kk < 2 * st_; ++kk) ur[(size_t)kk * dim + c] = uw[(size_t)c * 2 * st_ + kk];
    if (int rc = e->upload_w(&m->upsample_w, ur.data(), ur.size())) return rc;
    std::vector<const float*> ptrs;
    ptrs.push_back(reinterpret_cast<const float*>(m->rvq_first.codebooks[0].w));
    for (auto& cb : m->rvq_rest.codebooks) ptrs.push_back(reinterpret_cast<const float*>(cb.w));
    if (e->wmode != DsmDevice::W_MEASURE)  // a table of device pointers: per engine, never part of the arena
      if (int rc = e->upload(&m->emb_ptrs, ptrs.data(), ptrs.size())) return rc;
  }
  return 0;
}

int alloc_cat(DsmDevice* e, float** out, const ConvGeom& c, int B) {
  return e->dalloc(out, (size_t)B * (c.S + c.T_in) * c.in_c);
}

ConvStateDesc conv_desc(float* cat, const ConvGeom& c) {
  ConvStateDesc d;
  d.cat = cat;
  d.bstride = (long)(c.S + c.T_in) * c.in_c;
  d.S = c.S;
  d.T = c.T_in;
  d.C = c.in_c;
  d.replicate = c.replicate ? 1 : 0;
  return d;
}
void add_desc(std::vector<ConvStateDesc>& descs, float* cat, const ConvGeom& c) {  // a conv that carries frames between steps
  if (c.S > 0) descs.push_back(conv_desc(cat, c));
}

// The SEANet encoder chain's buffers for B items of r frames each; cat_init for n_init items (the clip path keeps every clip's
// PCM there and runs the chain one clip at a time).  descs: the list the streaming path's carried conv states are appended to;
// null where nothing is carried.  floats, if given, grows by what was allocated.
int alloc_seanet_enc(DsmDevice* e, SeanetEnc* s, const MimiW& w, int n_init, int B, int r, std::vector<ConvStateDesc>* descs,
                     size_t* floats = nullptr) {
  auto alloc = [&](float** out, size_t count) {
    if (floats) *floats += count;
    return e->dalloc(out, count);
  };
  auto cat = [&](float** out, const ConvGeom& c, int n) {
    const ConvGeom g = over_frames(c, r);
    if (int rc = alloc(out, (size_t)n * (g.S + g.T_in) * g.in_c)) return rc;
    if (descs) add_desc(*descs, *out, g);
    return 0;
  };
  if (int rc = cat(&s->cat_init, w.init_conv, n_init)) return rc;
  s->stages.resize(w.stages.size());
  for (size_t i = 0; i < w.stages.size(); ++i) {
    const MimiW::Stage& st = w.stages[i];
    if (int rc = alloc(&s->stages[i].y, (size_t)B * st.ra.T_in * r * st.ra.in_c)) return rc;
    if (int rc = cat(&s->stages[i].cat_ra, st.ra, B)) return rc;
    if (int rc = cat(&s->stages[i].cat_rb, st.rb, B)) return rc;
    if (int rc = cat(&s->stages[i].cat_down, st.down, B)) return rc;
  }
  return cat(&s->cat_final, w.final_conv, B);
}

int alloc_mimi_state(DsmDevice* e, MimiState* s, const MimiW& w, int B) {
  const dsm_mimi_config& cfg = w.cfg;
  if (int rc = alloc_seanet_enc(e, &s->enc, w, B, B, 1, &s->h_descs)) return rc;
  const int Tt = w.final_conv.T_out, d = cfg.dimension;
  if (int rc = alloc_act(e, &s->act, (size_t)B * Tt, d, cfg.transformer.dim_feedforward)) return rc;  // (hidden, or more with gating)
  if (int rc = alloc_cat(e, &s->cat_ds, w.downsample, B)) return rc;
  s->ds_desc = (int)s->h_descs.size();
  add_desc(s->h_descs, s->cat_ds, w.downsample);
  if (int rc = e->dalloc(&s->latent, (size_t)B * d)) return rc;
  if (int rc = e->dalloc(&s->res_first, (size_t)B * cfg.quantizer_dim)) return rc;
  if (int rc = e->dalloc(&s->res_rest, (size_t)B * cfg.quantizer_dim)) return rc;
  const int n_tiles = (cfg.quantizer_bins + 15) / 16;
  if (int rc = e->dalloc(&s->pval, (size_t)n_tiles * B)) return rc;
  if (int rc = e->dalloc(&s->pidx, (size_t)n_tiles * B)) return rc;
  if (int rc = e->dalloc(&s->codes, (size_t)B * cfg.quantizer_n_q)) return rc;
  if (int rc = e->dalloc(&s->mask, B)) return rc;
  if (int rc = alloc_transformer_state(e, &s->tr, cfg.transformer, B, Tt, false)) return rc;
  if (int rc = e->upload(&s->descs, s->h_descs.data(), s->h_descs.size())) return rc;
  s->pcm = s->enc.cat_init + (size_t)w.init_conv.S * w.init_conv.in_c;  // slot 0's frame; slots are bstride apart
  return 0;
}

// ----------------------------------------------------------------------------------------------
// GEMM launch
// ----------------------------------------------------------------------------------------------
// What launch_gemm hands back when it left the split-K slabs to the caller's next kernel: chunk c of row m starts at
// ws + c * cstride + m * ld.  ws is null when the product was reduced (or never split).
struct Slabs {
  const float* ws = nullptr;
  long ld = 0, cstride = 0;
  int chunks = 0;
};

// The main launch of a plan, for MT 16-row tiles per workgroup.  Every kernel form is instantiated for every MT it exists at;
// which one runs is the plan's (dsm_gemm_plan.h).
template <typename WT, typename KVT, int EPI, int NT, int MT>
void launch_form(const GemmPlan& p, hipStream_t st, const GemmArgs& a) {
  const dim3 grid(p.gx, p.gy, p.gz), block(p.block);
  switch (p.form) {
    case GEMM_MFMA:
      if (p.k_aligned) hipLaunchKernelGGL((gemm_mfma_kernel<WT, KVT, MT, NT, EPI, true>), grid, block, p.lds, st, a);
      else hipLaunchKernelGGL((gemm_mfma_kernel<WT, KVT, MT, NT, EPI, false>), grid, block, p.lds, st, a);
      break;
    case GEMM_MFMA_BX3:
      if (p.k_aligned) hipLaunchKernelGGL((gemm_mfma_kernel<WT, KVT, MT, NT, EPI, true, true>), grid, block, p.lds, st, a);
      else hipLaunchKernelGGL((gemm_mfma_kernel<WT, KVT, MT, NT, EPI, false, true>), grid, block, p.lds, st, a);
      break;
    case GEMM_TILE: hipLaunchKernelGGL((gemm_tile_kernel<WT, KVT, MT, NT, EPI>), grid, block, p.lds, st, a); break;
    case GEMM_LOOP2: hipLaunchKernelGGL((gemm_loop_kernel<WT, KVT, MT, NT, EPI, 2>), grid, block, p.lds, st, a); break;
    case GEMM_LOOP_DEEP: hipLaunchKernelGGL((gemm_loop_kernel<WT, KVT, MT, NT, EPI, LoopDepth<WT, NT>::MAX>), grid, block, p.lds, st, a); break;
    case GEMM_BX3_LOOP: hipLaunchKernelGGL((gemm_bx3_kernel<KVT, MT, NT, EPI, true>), grid, block, p.lds, st, a); break;
    case GEMM_BX3_LOOP_NT2:
      if constexpr (MT == 4)
        hipLaunchKernelGGL((gemm_bx3_kernel<KVT, 4, (NT == 1 ? 2 : NT), (EPI == EPI_GATE ? EPI_STORE : EPI), true>), grid, block, p.lds, st, a);
      break;
    case GEMM_BX3_SPLIT:
      if constexpr (MT == 4) hipLaunchKernelGGL((gemm_bx3_kernel<KVT, 4, NT, EPI, false>), grid, block, p.lds, st, a);
      break;
    case GEMM_BX3U_2:
      if constexpr (MT == 2) hipLaunchKernelGGL((gemm_bx3u_kernel<KVT, 2, NT, EPI, 8, 0, 4>), grid, block, p.lds, st, a);
      break;
    case GEMM_BX3U_1:
      if constexpr (MT == 1) hipLaunchKernelGGL((gemm_bx3u_kernel<KVT, 1, NT, EPI, 8>), grid, block, p.lds, st, a);
      break;
    case GEMM_WK:
      if constexpr (MT == 1 && EPI == EPI_GATE && NT == 2)
        hipLaunchKernelGGL((gemm_wk_kernel<KVT, 1, 2, EPI_GATE, 1, 4, 2, true, 4>), grid, block, p.lds, st, a);
      break;
    case GEMM_NO_FIT: break;
  }
}

// Y (and / or Y2, the row norm behind it) = epilogue(X W^T): fills a GemmQuery from the arguments, asks plan_gemm
// (dsm_gemm_plan.h) and executes the plan — the workspace, the main launch, the reduce, the row norm.  It decides nothing itself
// and does not write the caller's arguments.  slabs: non-null when the caller's next kernel can sum split-K slabs itself; its ws
// is non-null on return exactly when they were left to it.
// What plan_gemm is asked for a launch's arguments, and the knobs of the device context it is asked with: launch_gemm's own
// question, also put by dsm_debug_gemm before it launches (which epilogue a plan ends in decides what that aid can offer).
GemmQuery gemm_query(const GemmArgs& args, bool weight_bf16, int epi, int nt, bool aligned, bool may_defer) {
  auto ok4 = [](const RowMap& m) { return m.ld % 4 == 0 && m.bstride % 4 == 0; };
  GemmQuery q;
  q.weight_bf16 = weight_bf16;
  q.epi = epi;
  q.NT = nt;
  q.M = args.M; q.N = args.N; q.K = args.K; q.Kpad = args.Kpad;
  q.nt_stride = args.nt_stride;
  q.aligned = aligned;
  q.has_Y = args.Y != nullptr; q.has_Y2 = args.Y2 != nullptr; q.has_res = args.res != nullptr;
  q.has_bias = args.bias != nullptr; q.has_norm = args.norm_out != nullptr;
  q.y_ok4 = ok4(args.ymap); q.y2_ok4 = ok4(args.y2map); q.res_ok4 = ok4(args.rmap);
  q.y_bstride0 = args.ymap.bstride == 0;
  q.may_defer = may_defer;
  return q;
}
GemmKnobs gemm_knobs(const DsmDevice* e) {
  GemmKnobs k;
  k.dot_mode = e->dot_mode;
  k.chunk_loop_min_tiles = e->chunk_loop_min_tiles;
  k.smallk_min_tiles = e->smallk_min_tiles;
  k.smallk_mt = e->smallk_mt;
  k.loop_depth = e->loop_depth;
  return k;
}

template <typename WT, typename KVT, int EPI, int NT>
int launch_gemm(DsmDevice* e, hipStream_t st, const GemmArgs& args, bool aligned, Slabs* slabs = nullptr) {
  static_assert(EPI_STORE == GEMM_EPI_STORE && EPI_QKV == GEMM_EPI_QKV && EPI_GATE == GEMM_EPI_GATE && EPI_RVQ == GEMM_EPI_RVQ, "");
  static_assert(LoopDepth<uint16_t, 1>::MAX == 4 && LoopDepth<uint16_t, 2>::MAX == 2 && LoopDepth<float, 1>::MAX == 2, "plan_gemm's `deep`");
  const GemmPlan p = plan_gemm(gemm_query(args, sizeof(WT) == 2, EPI, NT, aligned, slabs != nullptr), gemm_knobs(e));
  if (p.form == GEMM_NO_FIT) {
    e->set_error("GEMM K=%d: chunk partials do not fit in LDS", args.K);
    return DSM_ERR_INVALID;
  }
  GemmArgs a = args;
  a.vec = p.vec;
  a.chunk_loop = p.chunk_loop;
  a.wg_cols = p.wg_cols;
  a.nt_stride = p.nt_stride;
  a.ws_ntiles = p.ws_ntiles;
  const int sid = e->sid(st);
  if (p.ws_bytes) {
    if (p.ws_bytes > e->gemm_ws_cap[sid]) {  // first use of a bigger shape: grow (never happens in steady state)
      if (e->capturing) {  // a graph capture cannot allocate: give up on this capture, the caller reruns the body eagerly
        e->capture_failed = true;
        e->set_error("split-K workspace grew during a graph capture");
        return DSM_ERR_STATE;
      }
      e->ws_gen += 1;
      HIPCHK(hipStreamSynchronize(st));
      if (e->gemm_ws[sid]) HIPCHK(hipFree(e->gemm_ws[sid]));
      e->gemm_ws[sid] = nullptr;
      e->gemm_ws_cap[sid] = 0;
      void* ws = nullptr;
      HIPCHK(hipMalloc(&ws, p.ws_bytes));
      e->gemm_ws[sid] = reinterpret_cast<float*>(ws);
      e->gemm_ws_cap[sid] = p.ws_bytes;
    }
    a.ws = e->gemm_ws[sid];
  }
  if (p.tiled) a.ts = e->timeline ? e->dev_ts_slot(e->tag_gemm[sid], sid, 1, 2) : nullptr;
  const int ph = e->prof_begin(e->tag_gemm[sid], st);
  switch (p.MT) {
    case 4: launch_form<WT, KVT, EPI, NT, 4>(p, st, a); break;
    case 2: launch_form<WT, KVT, EPI, NT, 2>(p, st, a); break;
    default: launch_form<WT, KVT, EPI, NT, 1>(p, st, a); break;
  }
  switch (p.reduce) {
    case GEMM_RED_NONE: case GEMM_RED_CONSUMER: break;
    case GEMM_RED_ROWS1: hipLaunchKernelGGL(gemm_reduce_rows_kernel<1>, dim3(a.M), dim3(256), 0, st, a, p.chunks); break;
    case GEMM_RED_ROWS2: hipLaunchKernelGGL(gemm_reduce_rows_kernel<2>, dim3(a.M), dim3(512), 0, st, a, p.chunks); break;
    case GEMM_RED_ROWS4: hipLaunchKernelGGL(gemm_reduce_rows_kernel<4>, dim3(a.M), dim3(1024), 0, st, a, p.chunks); break;
    case GEMM_RED_TILES: {
      const int out_tiles = ((a.M + 15) / 16) * ((a.N + 15) / 16);
      hipLaunchKernelGGL((gemm_reduce_kernel<KVT, EPI>), dim3((out_tiles + 3) / 4), dim3(256), 0, st, a, p.chunks);
      break;
    }
  }
  e->prof_end(ph, st);
  HIPCHK(hipGetLastError());
  if (p.row_norm) {
    // (a row wider than row_norm_kernel's registers hold: the two-pass form, same arithmetic)
    hipLaunchKernelGGL(a.N > 1024 * DSM_ROW_ITS ? row_norm_wide_kernel : row_norm_kernel, dim3(a.M), dim3(256), 0, st, a.norm_out, a.Y,
                       a.norm_w, a.norm_b, a.M, a.N, a.norm_eps, a.norm_rms);
    HIPCHK(hipGetLastError());
  }
  if (slabs) {
    *slabs = Slabs{};
    if (p.reduce == GEMM_RED_CONSUMER) {
      slabs->ws = a.ws;
      slabs->ld = (long)p.ws_ntiles * 16;
      slabs->cstride = (long)((a.M + 15) / 16) * 16 * slabs->ld;
      slabs->chunks = p.chunks;
    }
  }
  return 0;
}

// Run `body` (a sequence of launches on `st`) eagerly, or — once it has run twice with the same key — capture it into a
// hipGraph and replay that from then on.  key: everything the body's launch arguments depend on that may change between
// calls (caller-supplied pointers, branch selectors).
template <typename F>
int run_captured(DsmDevice* e, DsmDevice::GraphSlot& gs, hipStream_t st, uint64_t key, F&& body) {
  if (!e->use_graphs || e->prof_mask != 0 || gs.disabled) { e->eager_bodies += 1; return body(); }
  if (gs.exec && gs.key == key && gs.ws_gen == e->ws_gen) {
    HIPCHK(hipGraphLaunch(gs.exec, st));
    e->graph_launches += 1;
    return 0;
  }
  if (gs.key != key || gs.ws_gen != e->ws_gen) {  // new arguments: settle again before capturing
    gs.key = key;
    gs.ws_gen = e->ws_gen;
    gs.warm = 0;
    if (gs.exec) { (void)hipGraphExecDestroy(gs.exec); gs.exec = nullptr; }
  }
  if (gs.warm < 2) {
    gs.warm += 1;
    e->eager_bodies += 1;
    const int rc = body();
    if (gs.ws_gen != e->ws_gen) { gs.ws_gen = e->ws_gen; gs.warm = 0; }  // a workspace moved during this run
    return rc;
  }
  // Relaxed mode: the body only launches kernels and async copies on `st`; other threads are kept out by the API lock.
  ApiExclusive alone(e);
  hipError_t hb = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
  if (hb != hipSuccess) {
    (void)hipGetLastError();
    e->note_capture_failure("hipStreamBeginCapture", hb);
    if (++gs.failures >= DsmDevice::kMaxCaptureTries) gs.disabled = true;
    gs.warm = 0;
    e->eager_bodies += 1;
    return body();
  }
  e->capturing = true;
  e->capture_failed = false;
  const int rc = body();
  e->capturing = false;
  hipGraph_t g = nullptr;
  const hipError_t he = hipStreamEndCapture(st, &g);
  hipError_t hi = hipSuccess;
  if (!rc && he == hipSuccess && g) hi = hipGraphInstantiate(&gs.exec, g, nullptr, nullptr, 0);
  if (g) (void)hipGraphDestroy(g);
  if (rc || he != hipSuccess || !g || hi != hipSuccess) {
    // Never silent (r02 swallowed this and stayed eager for good): counted in dsm_metrics.capture_failures with the first
    // reason kept, the body re-run launch by launch so that the step still happens, and the capture tried again after two
    // more settled runs — up to kMaxCaptureTries times, then this sequence stays eager.
    gs.exec = nullptr;
    (void)hipGetLastError();
    e->note_capture_failure(rc ? (e->capture_failed ? "workspace grew during capture" : "launch error during capture")
                               : he != hipSuccess ? "hipStreamEndCapture" : !g ? "hipStreamEndCapture returned no graph" : "hipGraphInstantiate",
                            rc ? hipSuccess : he != hipSuccess ? he : hi);
    if (++gs.failures >= DsmDevice::kMaxCaptureTries) gs.disabled = true;
    gs.warm = 0;
    e->eager_bodies += 1;
    return body();
  }
  HIPCHK(hipGraphLaunch(gs.exec, st));
  e->graph_launches += 1;
  return 0;
}

RowMap plain_map(int M, int ld) {
  RowMap r;
  r.bstride = 0;
  r.rpb = M > 0 ? M : 1;
  r.ld = ld;
  r.toff = 0;
  return r;
}
RowMap batch_map(long bstride, int rpb, int ld, int toff) {
  RowMap r;
  r.bstride = bstride;
  r.rpb = rpb;
  r.ld = ld;
  r.toff = toff;
  return r;
}
RowMap cat_map(const ConvGeom& consumer) {  // rows (b, t) -> the consumer's concat buffer, after its carried frames
  return batch_map((long)(consumer.S + consumer.T_in) * consumer.in_c, consumer.T_in, consumer.in_c, consumer.S);
}

GemmArgs base_args(const Linear& L, const float* X, RowMap xmap, int M) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  a.X = X;
  a.xmap = xmap;
  a.W = L.w;
  a.wpacked = L.packed ? 1 : 0;
  a.Kpad = L.Kpad;
  a.K = L.K;
  a.N = L.N;
  a.M = M;
  a.nt_stride = 16;
  a.bias = L.bias;
  return a;
}

float norm_eps(int rms) { return rms ? 1e-8f : 1e-5f; }  // LayerNorm / RmsNorm — core/batched_transformer.rs:236-252

// the row norm behind this GEMM: out = norm(Y), fused into the split-K reduce where the plan can (gemm_reduce_rows_kernel)
void set_norm(GemmArgs& a, const float* w, const float* b, float* out, int rms) {
  a.norm_w = w;
  a.norm_b = b;
  a.norm_out = out;
  a.norm_eps = norm_eps(rms);
  a.norm_rms = rms;
}

template <typename WT>
int gemm_store(DsmDevice* e, hipStream_t st, const GemmArgs& a, bool aligned = true, Slabs* slabs = nullptr) {
  return launch_gemm<WT, float, EPI_STORE, 1>(e, st, a, aligned, slabs);
}

// conv as a GEMM over the consumer's concat buffer; output goes to Y (raw) and/or Y2 (ELU copy, usually the
// next conv's concat buffer at time offset S_next)
int run_conv(DsmDevice* e, hipStream_t st, const ConvGeom& c, const float* cat, int B, float* y, RowMap ymap,
             float* y2, RowMap y2map, const float* res, RowMap rmap) {
  const long bstride = (long)(c.S + c.T_in) * c.in_c;
  GemmArgs a = base_args(c.lin, cat, batch_map(bstride, c.T_out, c.stride * c.in_c, 0), B * c.T_out);
  a.Y = y;
  a.ymap = ymap;
  a.Y2 = y2;
  a.y2map = y2map;
  a.res = res;
  a.rmap = rmap;
  bool aligned = ((c.stride * c.in_c) % 4 == 0) && (bstride % 4 == 0);
  return gemm_store<float>(e, st, a, aligned);
}

}  // namespace

#include "dsm_engine_api.inc"
#include "dsm_slot_state.inc"
#include "dsm_text_bias.inc"
#include "dsm_ingest.inc"
#include "dsm_asr_clip.inc"
#include "dsm_tts.inc"
#include "dsm_tts_voice.inc"
#include "dsm_tts_slot_state.inc"
#include "dsm_tts_request.inc"
#include "dsm_egress.inc"
#include "dsm_speaker.inc"
#include "dsm_tts_cond.inc"
#include "dsm_audio.inc"
#include "dsm_worker.inc"
