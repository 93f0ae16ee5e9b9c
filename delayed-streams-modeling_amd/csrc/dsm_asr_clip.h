/*
 * dsm_asr_clip.h — a slot's CLIP: audio that is known beforehand, kept on the device in the slot's own ingest format
 * (dsm_pcm_format.h, DSM_PCM_IN) and cut into the slot's frames there, K steps per visit (dsm_asr_run / dsm_asr_collect,
 * dsm_asr_clip.inc).  ONE definition, host only, of what the device side has to do: the cut (asr_clip_frame_kernel, dsm_kernels.h,
 * copies the bytes this header names), the schedule (the [K][B] table dsm_asr_run uploads is plan()'s output) and the reader of
 * a block's records (dsm_asr_collect goes through unpack()).  The reference's request path (BatchedAsr::handle_query,
 * srv/batched_asr.rs:810-854) queues the decoded audio, then zeros, and cuts the queue into whole frames; this is that queue
 * with the audio left in the format it arrived in.
 *
 * THE CUT.  A slot's clip is clip_bytes bytes in the slot's format, frame_bytes = the format's frame (dsm_pcm_desc).  Frame i is
 * bytes [i frame_bytes, (i + 1) frame_bytes) of the clip FOLLOWED BY ENDLESS SILENCE.  The silence byte: 0x00 for DSM_PCM_F32 and
 * DSM_PCM_S16 (the sample 0), 0xFF for DSM_PCM_MULAW (expands to 0), 0xD5 for DSM_PCM_ALAW (the idle code; A-law has no zero, it
 * expands to +8).  A clip need not end on a sample: the silence starts at the byte behind it.
 *
 * THE SCHEDULE.  n_audio = ceil(clip_bytes / frame_bytes).  A CLOSED slot takes frames 0 .. n_audio + flush_frames - 1, one per
 * step, and is then DONE.  An OPEN slot takes frame i only once all of its bytes are there ((i + 1) frame_bytes <= clip_bytes);
 * otherwise it sits the step out with mask 0 and is WAITING until the next push or the close.  Nothing of it depends on data,
 * so the host knows every slot's frame index and mask for all K steps of a block when the block is enqueued.
 *
 *   state     begin -> RUNNING;  a step sat out (open) -> WAITING;  push / close on WAITING -> RUNNING;
 *             closed and every frame taken -> DONE;  dsm_asr_reset_slot -> IDLE
 *
 * THE RECORDS of a block of n steps, one row of B (2 + heads) u32 words per step: text token [B], log-probability [B] (the
 * quiet NaN 0x7FC00000 while token scores are off), VAD values [heads][B].
 */
#ifndef DSM_ASR_CLIP_H
#define DSM_ASR_CLIP_H

#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/dsm.h"
#include "dsm_pcm_format.h"

namespace dsm_asr_clip {

/* the byte a frame is filled with behind the clip's end */
inline uint8_t silence_byte(uint32_t fmt) { return fmt == DSM_PCM_MULAW ? 0xFFu : fmt == DSM_PCM_ALAW ? 0xD5u : 0x00u; }

/* frame `index` of a clip of clip_bytes bytes cut into frames of frame_bytes >= 1: frame_bytes bytes to `out`.  clip may be NULL
 * when clip_bytes is 0.  Returns how many of them came from the clip. */
inline size_t cut(const void* clip, uint64_t clip_bytes, uint32_t frame_bytes, uint8_t silence, uint64_t index, void* out) {
  uint64_t have = 0;
  if (index <= clip_bytes / frame_bytes) {  /* index * frame_bytes <= clip_bytes: no overflow */
    const uint64_t off = index * (uint64_t)frame_bytes;
    have = clip_bytes - off < frame_bytes ? clip_bytes - off : frame_bytes;
    if (have) memcpy(out, (const uint8_t*)clip + off, (size_t)have);
  }
  memset((uint8_t*)out + have, silence, (size_t)(frame_bytes - have));
  return (size_t)have;
}

/* one slot's clip as the schedule sees it */
struct Slot {
  int status = DSM_ASR_CLIP_IDLE;
  bool closed = false;
  uint32_t frame_bytes = 0;
  uint64_t bytes = 0;    /* pushed so far */
  uint64_t cursor = 0;   /* the next frame's index */
  uint64_t flush = 0;    /* silent frames behind the audio */
};

inline uint64_t n_audio(const Slot& s) { return s.bytes / s.frame_bytes + (s.bytes % s.frame_bytes ? 1u : 0u); }

inline void begin(Slot* s, uint32_t frame_bytes, uint64_t flush_frames) {
  *s = Slot();
  s->status = DSM_ASR_CLIP_RUNNING;
  s->frame_bytes = frame_bytes;
  s->flush = flush_frames;
}

/* false, nothing changed: no open clip, or the clip would pass `cap` bytes */
inline bool push(Slot* s, uint64_t n, uint64_t cap) {
  if (s->status == DSM_ASR_CLIP_IDLE || s->closed || n > cap || s->bytes > cap - n) return false;
  s->bytes += n;
  if (s->status == DSM_ASR_CLIP_WAITING) s->status = DSM_ASR_CLIP_RUNNING;
  return true;
}

inline bool close(Slot* s) {
  if (s->status == DSM_ASR_CLIP_IDLE) return false;
  if (s->closed) return true;
  s->closed = true;
  s->status = s->cursor >= n_audio(*s) + s->flush ? DSM_ASR_CLIP_DONE : DSM_ASR_CLIP_RUNNING;
  return true;
}

/* one step of the slot: true and *frame = the frame it takes, or false — it sits the step out (idle, done, or waiting) */
inline bool step(Slot* s, uint64_t* frame) {
  if (s->status == DSM_ASR_CLIP_IDLE || s->status == DSM_ASR_CLIP_DONE || s->frame_bytes == 0) return false;
  if (s->closed) {
    const uint64_t total = n_audio(*s) + s->flush;
    if (s->cursor >= total) { s->status = DSM_ASR_CLIP_DONE; return false; }
    *frame = s->cursor++;
    if (s->cursor >= total) s->status = DSM_ASR_CLIP_DONE;
    return true;
  }
  if (s->cursor >= s->bytes / s->frame_bytes) { s->status = DSM_ASR_CLIP_WAITING; return false; }
  *frame = s->cursor++;
  return true;
}

/* the block's table: n_steps steps of B slots, frame [n_steps][B] and mask [n_steps][B]; the slots advance */
inline void plan(Slot* slots, int B, int n_steps, uint32_t* frame, uint8_t* mask) {
  for (int k = 0; k < n_steps; ++k)
    for (int b = 0; b < B; ++b) {
      uint64_t f = 0;
      const bool on = step(&slots[b], &f);
      frame[(size_t)k * B + b] = on ? (uint32_t)f : 0u;  /* a clip of at most 2^31 bytes plus a flush below 2^31 frames: fits */
      mask[(size_t)k * B + b] = on ? 1u : 0u;
    }
}

/* words of one step's record row */
inline size_t record_words(int B, int heads) { return (size_t)B * (2u + (size_t)heads); }

/* Step k of a record buffer of rec_words words holding n_steps rows: its three arrays, or false when the row does not lie
 * inside the buffer (n_steps 1 .. DSM_ASR_RUN_MAX, 0 <= k < n_steps, B >= 1, 0 <= heads <= DSM_MAX_EXTRA_HEADS). */
inline bool record_row(const uint32_t* rec, size_t rec_words, int n_steps, int B, int heads, int k, const uint32_t** text,
                       const uint32_t** logprob, const uint32_t** prs) {
  if (!rec || n_steps < 1 || n_steps > DSM_ASR_RUN_MAX || k < 0 || k >= n_steps || B < 1 || heads < 0 || heads > DSM_MAX_EXTRA_HEADS)
    return false;
  const size_t row = record_words(B, heads);
  if (rec_words / row < (size_t)n_steps) return false;
  const uint32_t* r = rec + (size_t)k * row;
  *text = r;
  *logprob = r + B;
  *prs = r + 2 * (size_t)B;
  return true;
}

/* A block's records into the caller's arrays (any may be NULL): stepped [n][B] from the table's masks, text_token [n][B],
 * vad_prs [n][heads][B], logprob [n][B].  False, nothing written, when the records do not hold n_steps rows. */
inline bool unpack(const uint32_t* rec, size_t rec_words, const uint8_t* mask, int n_steps, int B, int heads, uint8_t* stepped,
                   uint32_t* text_token, float* vad_prs, float* logprob) {
  const uint32_t *t = nullptr, *l = nullptr, *p = nullptr;
  if (!mask || !record_row(rec, rec_words, n_steps, B, heads, n_steps - 1, &t, &l, &p)) return false;
  for (int k = 0; k < n_steps; ++k) {
    record_row(rec, rec_words, n_steps, B, heads, k, &t, &l, &p);
    if (stepped) memcpy(stepped + (size_t)k * B, mask + (size_t)k * B, (size_t)B);
    if (text_token) memcpy(text_token + (size_t)k * B, t, sizeof(uint32_t) * (size_t)B);
    if (logprob) memcpy(logprob + (size_t)k * B, l, sizeof(uint32_t) * (size_t)B);
    if (vad_prs && heads > 0) memcpy(vad_prs + (size_t)k * heads * B, p, sizeof(uint32_t) * (size_t)heads * B);
  }
  return true;
}

/* The messages of step k of a block (what assemble_words left for that step: n_msgs messages, their n_toks tokens and the
 * tokens' log-probabilities) behind those of the steps before it in the caller's arrays: a Word's tokens_offset is rebased on
 * the block's first token; what lies beyond msgs_cap / tokens_cap is counted and dropped. */
inline void append_step(dsm_asr_block* out, int k, const dsm_asr_msg* msgs, size_t n_msgs, const uint32_t* toks, const float* lps,
                        size_t n_toks) {
  for (size_t i = 0; i < n_msgs; ++i) {
    if (out->n_msgs < out->msgs_cap) {
      dsm_asr_msg c = msgs[i];
      if (c.kind == DSM_MSG_WORD) {
        const int64_t at = (int64_t)c.tokens_offset + out->n_tokens;
        c.tokens_offset = at > INT32_MAX ? INT32_MAX : (int)at;
      }
      out->msgs[out->n_msgs] = c;
      out->msg_step[out->n_msgs] = k;
    }
    if (out->n_msgs < INT32_MAX) out->n_msgs += 1;
  }
  for (size_t i = 0; i < n_toks; ++i) {
    if (out->n_tokens < out->tokens_cap) {
      out->msg_tokens[out->n_tokens] = toks[i];
      out->msg_logprobs[out->n_tokens] = lps[i];
    }
    if (out->n_tokens < INT32_MAX) out->n_tokens += 1;
  }
}

}  // namespace dsm_asr_clip

#endif /* DSM_ASR_CLIP_H */
