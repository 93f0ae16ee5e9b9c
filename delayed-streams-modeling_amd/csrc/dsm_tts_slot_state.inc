// dsm_tts_slot_state.inc — the TTS slot blob's entry point (included by dsm_engine.hip behind dsm_tts_voice.inc).  The format,
// its writer and its checked reader are csrc/dsm_tts_slot_blob.h over the container of csrc/dsm_slot_blob.h, host only; DESIGN.md section 7.2 has the table of state the
// blob is laid out for.  The engine calls that fill and consume a blob (export / import) are not in the library yet.

extern "C" {

int dsm_tts_slot_blob_info(const void* buf, size_t len, struct dsm_tts_slot_blob_info* out) {
  std::string err;
  const int rc = dsm_tts_slot_blob::info(buf, len, out, &err);
  if (rc) g_create_error = err;  // no engine is involved: dsm_tts_last_error(NULL), like a failed create
  return rc;
}

}  // extern "C"
