// dsm_tts_cond.inc — ConditionProvider (core/conditioner.rs:31-176) for the TTS engine: LUT and continuous-attribute conditioners
// per slot (part of the library's one translation unit, beside dsm_speaker.inc).  The reference's server builds ONE
// Condition::AddToInput per request (srv/tts.rs:416-423: condition_lut("control", "also_good")) and hands it to every State::step;
// LmModel::forward_cond / forward_ca add it to the input embedding sum of every batch row (core/lm.rs:996-1000, :1062-1066).
// Here a slot's row is computed once per dsm_tts_set_condition_* call by tts_cond_row_kernel into d_cond[slot] (f32: the
// reference's final rounding of the projected row to the checkpoint dtype is NOT applied, like the speaker rows) and
// tts_input_kernel adds it behind the per-slot flag.  Both buffers exist from dsm_tts_create on, so the captured step bodies —
// and the K-steps-per-visit loop of dsm_tts_run, which replays them — see a condition without recapture.
//
// The calls run on the model stream between steps and wait for it, like dsm_tts_set_ca_src.

namespace {

enum { TTS_COND_SET_LUT = 0, TTS_COND_SET_CONT = 1, TTS_COND_SET_PADDING = 2 };

// One tensor as f32 with its shape checked (BF16 is upcast exactly).  `shape` has ndim entries.
int cond_read(DsmDevice* e, const dsm_st_file* f, const std::string& key, const int64_t* shape, int ndim, std::vector<float>& out) {
  char err[512];
  const dsm_st_tensor* tp = dsm_st_find(f, key.c_str());
  if (!tp) { e->set_error("cannot find tensor %s", key.c_str()); return DSM_ERR_IO; }
  bool same = tp->ndim == ndim;
  int64_t numel = 1;
  for (int i = 0; i < ndim; ++i) {
    same = same && tp->shape[i] == shape[i];
    numel *= shape[i];
  }
  if (!same) {
    std::string want;
    for (int i = 0; i < ndim; ++i) want += "[" + std::to_string((long long)shape[i]) + "]";
    e->set_error("shape mismatch for %s: expected %s", key.c_str(), want.c_str());
    return DSM_ERR_IO;
  }
  out.resize((size_t)numel);
  if (dsm_st_read_f32(f, key.c_str(), numel, out.data(), err, sizeof err)) { e->set_error("%s", err); return DSM_ERR_IO; }
  return 0;
}

int cond_check_desc(DsmDevice* e, const dsm_tts_conditioner_desc* descs, int n) {
  for (int i = 0; i < n; ++i) {
    const dsm_tts_conditioner_desc& c = descs[i];
    if (!c.name || !c.name[0]) { e->set_error("conditioner %d has no name", i); return DSM_ERR_INVALID; }
    for (int j = 0; j < i; ++j)
      if (!strcmp(descs[j].name, c.name)) { e->set_error("conditioner %s is listed twice", c.name); return DSM_ERR_INVALID; }
    if (c.dim < 1 || c.dim > 65536) { e->set_error("conditioner %s: dim %d out of range", c.name, c.dim); return DSM_ERR_INVALID; }
    if (c.type == DSM_TTS_COND_LUT) {
      if (c.n_bins < 0 || c.n_values < 1 || !c.possible_values || c.n_values > c.n_bins + 1) {
        e->set_error("conditioner %s: a LUT needs 1 .. n_bins + 1 possible_values (n_bins %d, %d values)", c.name, c.n_bins, c.n_values);
        return DSM_ERR_INVALID;
      }
      for (int v = 0; v < c.n_values; ++v)
        if (!c.possible_values[v]) { e->set_error("conditioner %s: possible_values[%d] is null", c.name, v); return DSM_ERR_INVALID; }
    } else if (c.type == DSM_TTS_COND_CONTINUOUS) {
      // half_dim - 1 divides in create_sin_embeddings (core/conditioner.rs:93): dim 2 would be 0 / 0 there
      if (c.dim < 4 || c.dim % 2) { e->set_error("conditioner %s: a continuous attribute needs an even dim of at least 4 (got %d)", c.name, c.dim); return DSM_ERR_INVALID; }
      if (!(c.max_period > 0.0f) || !std::isfinite(c.max_period) || !std::isfinite(c.scale_factor)) {
        e->set_error("conditioner %s: max_period must be positive and scale_factor finite", c.name);
        return DSM_ERR_INVALID;
      }
    } else {
      e->set_error("conditioner %s: type %d is neither DSM_TTS_COND_LUT nor DSM_TTS_COND_CONTINUOUS", c.name, c.type);
      return DSM_ERR_INVALID;
    }
  }
  return 0;
}

int cond_attach_impl(dsm_tts* t, const dsm_tts_conditioner_desc* descs, int n, const char* lm_path) {
  DsmDevice* e = t;
  const int d = t->cfg.lm.d_model;
  if (int rc = cond_check_desc(e, descs, n)) return rc;
  char err[512];
  dsm_st_file* f = dsm_st_open(lm_path, err, sizeof err);
  if (!f) { e->set_error("%s", err); return DSM_ERR_IO; }
  // every tensor to the host first: a missing key or a wrong shape leaves the engine as it was
  struct Host { std::vector<float> embed, proj, pad; };
  std::vector<Host> host((size_t)n);
  int rc = 0, max_dim = 0;
  for (int i = 0; i < n && !rc; ++i) {
    const dsm_tts_conditioner_desc& c = descs[i];
    const std::string p = std::string("condition_provider.conditioners.") + c.name + ".";
    const int64_t s_embed[2] = {c.n_bins + 1, c.dim}, s_proj[2] = {d, c.dim}, s_pad[3] = {1, 1, d};
    if (c.type == DSM_TTS_COND_LUT) rc = cond_read(e, f, p + "embed.weight", s_embed, 2, host[i].embed);
    if (!rc) rc = cond_read(e, f, p + "output_proj.weight", s_proj, 2, host[i].proj);
    if (!rc) rc = cond_read(e, f, p + "learnt_padding", s_pad, 3, host[i].pad);
    if (c.dim > max_dim) max_dim = c.dim;
  }
  dsm_st_close(f);
  if (rc) return rc;
  TtsCond cp;
  for (int i = 0; i < n; ++i) {
    const dsm_tts_conditioner_desc& c = descs[i];
    TtsCond::One o;
    o.name = c.name; o.type = c.type; o.dim = c.dim;
    o.scale_factor = c.scale_factor; o.max_period = c.max_period;
    if (c.type == DSM_TTS_COND_LUT) {
      for (int v = 0; v < c.n_values; ++v) o.values.emplace_back(c.possible_values[v]);
      if ((rc = e->upload(&o.embed, host[i].embed.data(), host[i].embed.size()))) return rc;
    }
    if ((rc = e->upload(&o.proj, host[i].proj.data(), host[i].proj.size()))) return rc;
    if ((rc = e->upload(&o.pad, host[i].pad.data(), host[i].pad.size()))) return rc;
    cp.list.push_back(std::move(o));
  }
  if ((rc = e->dalloc(&cp.d_in, (size_t)max_dim))) return rc;
  HIPCHK(hipDeviceSynchronize());
  t->cond = std::move(cp);
  return 0;
}

// condition_lut / condition_cont / learnt_padding for one slot: checks, then ONE launch of tts_cond_row_kernel.
int cond_set_impl(dsm_tts* t, int slot, const char* name, int kind, const char* value, float fvalue) {
  DsmDevice* e = t;
  const int d = t->cfg.lm.d_model;
  if (t->cond.list.empty()) { e->set_error("no conditioners attached (dsm_tts_attach_conditioners first)"); return DSM_ERR_INVALID; }
  const TtsCond::One* c = nullptr;
  for (const TtsCond::One& o : t->cond.list)
    if (o.name == name) c = &o;
  if (!c) { e->set_error("unknown conditioner %s", name); return DSM_ERR_INVALID; }
  int idx = -1;
  if (kind == TTS_COND_SET_LUT) {
    if (c->type != DSM_TTS_COND_LUT) { e->set_error("cannot use conditioner with a str value %s", name); return DSM_ERR_INVALID; }
    for (size_t v = 0; v < c->values.size(); ++v)  // a HashMap built in list order: of equal strings the last position stays
      if (c->values[v] == value) idx = (int)v;
    if (idx < 0) { e->set_error("unknown value for lut conditioner '%s'", value); return DSM_ERR_INVALID; }
  } else if (kind == TTS_COND_SET_CONT) {
    if (c->type != DSM_TTS_COND_CONTINUOUS) { e->set_error("cannot use conditioner with a float value %s", name); return DSM_ERR_INVALID; }
    if (!std::isfinite(fvalue)) { e->set_error("conditioner %s: the value is not finite", name); return DSM_ERR_INVALID; }
  }
  // One Condition per State, fixed at its first step (srv/tts.rs:416-441): only a fresh slot takes one, as with dsm_tts_set_ca_src
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  if (t->items[slot].step_idx != 0) {
    e->set_error("slot %d is at step %zu: a condition needs a fresh slot (dsm_tts_reset_slot first)", slot, t->items[slot].step_idx);
    return DSM_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  const float *in = nullptr, *W = c->proj;
  std::vector<float> emb;
  if (kind == TTS_COND_SET_LUT) {
    in = c->embed + (size_t)idx * c->dim;
  } else if (kind == TTS_COND_SET_CONT) {
    // create_sin_embeddings (core/conditioner.rs:88-99) on the HOST, in double: dim values per request are not worth a kernel,
    // and the device side then only sees the bf16 values the reference's .to_dtype(output_proj.dtype()) would hand to the
    // projection (round to nearest even, dsm_numerics.h).  Cosines first.
    const int half = c->dim / 2;
    const double v = (double)fvalue * (double)c->scale_factor;
    emb.resize((size_t)c->dim);
    for (int i = 0; i < half; ++i) {
      const double a = 1.0 / pow((double)c->max_period, (double)i / (double)(half - 1));
      emb[i] = dsm_bf16_to_f32(dsm_f32_to_bf16((float)cos(v * a)));
      emb[half + i] = dsm_bf16_to_f32(dsm_f32_to_bf16((float)sin(v * a)));
    }
    HIPCHK(hipMemcpyAsync(t->cond.d_in, emb.data(), sizeof(float) * emb.size(), hipMemcpyHostToDevice, st));
    in = t->cond.d_in;
  } else {
    in = c->pad;
    W = nullptr;
  }
  hipLaunchKernelGGL(tts_cond_row_kernel, dim3((d + 255) / 256), dim3(256), 0, st, t->d_cond + (size_t)slot * d, t->d_cond_on + slot, in, W,
                     d, c->dim);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));  // `emb` is this call's memory
  t->cond_on[slot] = 1;
  return 0;
}

int cond_args(dsm_tts* t, int slot, const void* a, const void* b) {
  if (!t) { g_create_error = "null argument"; return DSM_ERR_INVALID; }
  if (slot < 0 || slot >= t->B || !a || !b) { t->set_error("condition: null argument or slot %d outside 0..%d", slot, t->B - 1); return DSM_ERR_INVALID; }
  return 0;
}

}  // namespace

extern "C" {

int dsm_tts_attach_conditioners(dsm_tts* t, const dsm_tts_conditioner_desc* descs, int n, const char* lm_safetensors) {
  if (!t) { g_create_error = "null argument"; return DSM_ERR_INVALID; }
  DsmDevice* e = t;
  if (!descs || !lm_safetensors || n < 1) { e->set_error("dsm_tts_attach_conditioners: null argument or no conditioner"); return DSM_ERR_INVALID; }
  if (!t->cond.list.empty()) { e->set_error("conditioners are attached already"); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // allocations (null-stream fills) must not run beside a capture
  HIPCHK(hipDeviceSynchronize());
  return cond_attach_impl(t, descs, n, lm_safetensors);
}

int dsm_tts_set_condition_lut(dsm_tts* t, int slot, const char* name, const char* value) {
  if (int rc = cond_args(t, slot, name, value)) return rc;
  return cond_set_impl(t, slot, name, TTS_COND_SET_LUT, value, 0.0f);
}

int dsm_tts_set_condition_cont(dsm_tts* t, int slot, const char* name, float value) {
  if (int rc = cond_args(t, slot, name, name)) return rc;
  return cond_set_impl(t, slot, name, TTS_COND_SET_CONT, nullptr, value);
}

int dsm_tts_set_condition_padding(dsm_tts* t, int slot, const char* name) {
  if (int rc = cond_args(t, slot, name, name)) return rc;
  return cond_set_impl(t, slot, name, TTS_COND_SET_PADDING, nullptr, 0.0f);
}

int dsm_tts_clear_condition(dsm_tts* t, int slot) {
  if (int rc = cond_args(t, slot, t, t)) return rc;
  DsmDevice* e = t;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  // stream-ordered: behind the steps already enqueued (a block that waits for dsm_tts_collect keeps its condition)
  HIPCHK(hipMemsetAsync(t->d_cond_on + slot, 0, 1, st));
  HIPCHK(hipMemsetAsync(t->d_cond + (size_t)slot * t->cfg.lm.d_model, 0, sizeof(float) * (size_t)t->cfg.lm.d_model, st));
  HIPCHK(hipStreamSynchronize(st));
  t->cond_on[slot] = 0;
  return 0;
}

}  // extern "C"
