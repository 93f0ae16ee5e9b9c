// dsm_tts_slot_state.inc — the TTS slot blob's host-only entry points (included by dsm_engine.hip behind dsm_tts_voice.inc).  The
// format, its writer and its checked reader are csrc/dsm_tts_slot_blob.h over the container of csrc/dsm_slot_blob.h; the payload's
// section list, the signature and the index checks an import has to make are csrc/dsm_tts_slot_layout.h, a function of the
// configuration alone; DESIGN.md section 7.2 has the table of state the blob is laid out for.  The engine calls that fill and
// consume a blob (export / import / move / fork) are not in the library: DESIGN.md section 7.2 says what happened to them.

extern "C" {

int dsm_tts_slot_blob_info(const void* buf, size_t len, struct dsm_tts_slot_blob_info* out) {
  std::string err;
  const int rc = dsm_tts_slot_blob::info(buf, len, out, &err);
  if (rc) g_create_error = err;  // no engine is involved: dsm_tts_last_error(NULL), like a failed create
  return rc;
}

int dsm_tts_slot_layout(const dsm_tts_config* cfg, const dsm_mimi_config* mimi, char* buf, size_t cap) {
  if (!cfg) { g_create_error = "null argument"; return DSM_ERR_INVALID; }
  dsm_tts_layout::Layout L;
  std::string err;
  if (!dsm_tts_layout::build(*cfg, mimi, &L, &err)) { g_create_error = "slot layout: " + err; return DSM_ERR_INVALID; }
  const std::string text = dsm_tts_layout::print(L);
  if (buf && cap > text.size()) memcpy(buf, text.c_str(), text.size() + 1);
  return (int)text.size();
}

}  // extern "C"
