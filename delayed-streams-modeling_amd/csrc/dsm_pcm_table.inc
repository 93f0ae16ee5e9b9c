// dsm_pcm_table.inc — PcmFormatTable: the formats of one engine's slots in one direction (csrc/dsm_pcm_format.h), as the resample
// kernels read them.  dsm_engine holds one (DSM_PCM_IN, dsm_ingest.inc), dsm_tts holds one (DSM_PCM_OUT, dsm_egress.inc); both
// are a DsmDevice, whose dalloc / set_error the table uses.  On the device: the descriptors [kFormats] (entry 0 = 24000 / F32,
// append-only: one per (rate, format) ever set), the coefficient arena (append-only: one phase table per rate) and each slot's
// descriptor index [B].  On the host: mirrors of the descriptors and of the indices.  The table locks nothing: its owner's rules
// hold (allocations and new entries under the exclusive side of api_mu; dsm_engine's mirrors under ingest_mu as well).

struct PcmFormatTable {
  static constexpr size_t kFormats = 64, kCoefWords = (size_t)1 << 20;
  const int dir;
  bool ready = false;  // ensure() has run to its end: set last, so the owner's own buffers come before it
  dsm_pcm_desc* descs_d = nullptr;
  float* coef_d = nullptr;
  uint32_t* slot_desc_d = nullptr;
  std::vector<dsm_pcm_desc> descs_h;
  std::vector<uint32_t> slot_desc_h;
  size_t coef_used = 0;

  explicit PcmFormatTable(int dir_) : dir(dir_) {}

  // the table's own allocations, every slot on entry 0, the pass-through format
  int ensure(DsmDevice* e, size_t B) {
    if (ready) return 0;
    if (int rc = e->dalloc(&descs_d, kFormats)) return rc;
    if (int rc = e->dalloc(&coef_d, kCoefWords, false)) return rc;
    if (int rc = e->dalloc(&slot_desc_d, B)) return rc;  // zeroed
    dsm_pcm_desc d0;
    std::string err;
    if (dsm_pcm::describe(dir, DSM_PCM_RATE, DSM_PCM_F32, &d0, &err)) { e->set_error("%s", err.c_str()); return DSM_ERR_INVALID; }
    HIPCHK(hipMemcpy(descs_d, &d0, sizeof d0, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    descs_h.assign(1, d0);
    slot_desc_h.assign(B, 0u);
    coef_used = 0;
    ready = true;
    return 0;
  }

  // the entry of (rate, fmt), made if it is new: the rate's phase table appended to the arena, the descriptor to the table.  New
  // entries are referenced by no slot, so no step in flight reads them: plain blocking copies.
  int entry(DsmDevice* e, int rate, int fmt, uint32_t* index) {
    dsm_pcm_desc d;
    std::string err;
    if (int rc = dsm_pcm::describe(dir, rate, fmt, &d, &err)) { e->set_error("%s", err.c_str()); return rc; }
    bool have_table = d.table_words == 0;
    for (size_t i = 0; i < descs_h.size(); ++i) {
      const dsm_pcm_desc& o = descs_h[i];
      if (o.rate == d.rate && o.fmt == d.fmt) { *index = (uint32_t)i; return 0; }
      if (o.rate == d.rate && !have_table) { d.table_off = o.table_off; have_table = true; }
    }
    const char* s = dsm_pcm::side(dir);
    if (descs_h.size() >= kFormats) {
      e->set_error("%s format: %d distinct formats are in use, no room for another", s, (int)kFormats);
      return DSM_ERR_STATE;
    }
    if (!have_table) {
      std::vector<float> ph;
      if (dsm_pcm::rate_table(dir, rate, nullptr, nullptr, nullptr, &ph) || ph.size() != d.table_words) {
        e->set_error("%s format: no phase table for %d Hz", s, rate);
        return DSM_ERR_INVALID;
      }
      if (coef_used + ph.size() > kCoefWords) {
        e->set_error("%s format: the coefficient arena is full (%zu of %zu words), no room for %d Hz", s, coef_used, kCoefWords, rate);
        return DSM_ERR_STATE;
      }
      d.table_off = (uint32_t)coef_used;
      HIPCHK(hipMemcpy(coef_d + d.table_off, ph.data(), sizeof(float) * ph.size(), hipMemcpyHostToDevice));
      coef_used += ph.size();
    }
    if (int rc = dsm_pcm::check(dir, &d, coef_used, &err)) { e->set_error("%s", err.c_str()); return rc; }
    const size_t at = descs_h.size();
    HIPCHK(hipMemcpy(descs_d + at, &d, sizeof d, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    descs_h.push_back(d);
    *index = (uint32_t)at;
    return 0;
  }

  const dsm_pcm_desc& slot(int b) const { return descs_h[slot_desc_h[(size_t)b]]; }

  // a slot's index, on the device and in the mirror: blocking.  Frames in flight read the word: the owner drains its streams first.
  int set_slot(DsmDevice* e, int b, uint32_t index) {
    HIPCHK(hipMemcpy(slot_desc_d + b, &index, sizeof index, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    slot_desc_h[(size_t)b] = index;
    return 0;
  }

  // what dsm_asr_input_format / dsm_tts_output_format answer: the slot's format — the pass-through format while the section
  // has never been turned on
  int get(int b, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples) const {
    dsm_pcm_desc d;
    if (ready) d = slot(b);
    else {
      std::string err;
      if (int rc = dsm_pcm::describe(dir, DSM_PCM_RATE, DSM_PCM_F32, &d, &err)) return rc;
    }
    if (rate) *rate = (int)d.rate;
    if (fmt) *fmt = (int)d.fmt;
    if (frame_samples) *frame_samples = (int)d.frame;
    if (frame_bytes) *frame_bytes = (int)d.frame_bytes;
    if (latency_samples) *latency_samples = (int)d.D;
    return 0;
  }

  // a raw call's pitch: non-zero, a multiple of 16, at most 15360, and at least the frame_bytes of every slot that counts — the
  // slots `marks` marks, or every slot with `all`
  int check_pitch(DsmDevice* e, size_t pitch, const uint8_t* marks, bool all) const {
    if (pitch == 0 || pitch % 16 != 0 || pitch > DSM_PCM_MAX_FRAME_BYTES) {
      e->set_error("raw frames: a pitch of %zu bytes (a multiple of 16, at most %u)", pitch, DSM_PCM_MAX_FRAME_BYTES);
      return DSM_ERR_INVALID;
    }
    for (int b = 0; b < (int)slot_desc_h.size(); ++b) {
      if (!all && !(marks && marks[b])) continue;
      const dsm_pcm_desc& d = slot(b);
      if (d.frame_bytes > pitch) {
        e->set_error("raw frames: slot %d's frame has %u bytes, the pitch is %zu", b, d.frame_bytes, pitch);
        return DSM_ERR_INVALID;
      }
    }
    return 0;
  }
};
