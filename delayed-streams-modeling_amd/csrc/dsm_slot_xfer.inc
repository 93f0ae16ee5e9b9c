// dsm_slot_xfer.inc — moving slot state between an engine's buffers and a staging buffer: the section table, its device copy,
// the staging buffers, the pack / unpack launch (slot_state_pack_kernel / slot_state_unpack_kernel, dsm_kernels.h) and the
// checks that know no model.  Included by dsm_engine.hip behind dsm_kernels.h; everything is a function of a DsmDevice and a
// SlotXfer, so either engine can hold one.  What the sections are, the signature and the host items are the engine's
// (dsm_slot_state.inc for the STT engine).  A slot's payload is a base group of sections plus one optional tail group that a
// blob may lack and an engine may not have yet (STT: LM + mimi[0], then mimi[1]).

namespace {

struct SlotXfer {
  std::mutex mu;                    // one export / import / move per engine at a time
  std::vector<SlotSection> secs;    // base group, then the optional group, whose bases stay null until it exists
  std::vector<uint32_t> sig;        // the blob signature of this configuration
  int nsec_base = 0, nsec_opt = 0;
  unsigned chunks_base = 0, chunks_opt = 0;
  size_t bytes_base = 0, bytes_opt = 0;
  SlotSection* d_secs = nullptr;
  bool d_has_opt = false;           // the device table holds the optional group's bases
  char* d_stage = nullptr;
  size_t d_stage_cap = 0;
  char* h_stage = nullptr;          // pinned
  size_t h_stage_cap = 0;
  int* d_slots = nullptr;
  int slots_cap = 0;
  hipEvent_t ev_packed = nullptr;
};

// Payload offsets, piece counts and the totals of both groups for the sections `v`, of which the first nsec_base are the base group.
void slot_layout_finish(SlotXfer& x, std::vector<SlotSection> v, int nsec_base) {
  x.nsec_base = nsec_base;
  x.nsec_opt = (int)v.size() - nsec_base;
  long off = 0;
  unsigned chunk = 0;
  for (int i = 0; i < (int)v.size(); ++i) {
    if (i == nsec_base) {
      x.bytes_base = (size_t)off;
      x.chunks_base = chunk;
    }
    v[i].off = off;
    v[i].chunk0 = chunk;
    off += (long)dsm_blob::align16((uint64_t)v[i].bytes);
    chunk += (unsigned)((v[i].bytes + kSlotChunk - 1) / kSlotChunk);
  }
  x.bytes_opt = (size_t)off - x.bytes_base;
  x.chunks_opt = chunk - x.chunks_base;
  x.secs = std::move(v);
}

// First difference between two signatures, as text (name_of: what word i of a signature stands for); empty when they agree.
std::string slot_sig_mismatch(const uint32_t* theirs, size_t n_theirs, const std::vector<uint32_t>& ours, const char* (*name_of)(size_t)) {
  char buf[160];
  for (size_t i = 0; i < ours.size() && i < n_theirs; ++i)
    if (theirs[i] != ours[i]) {
      snprintf(buf, sizeof buf, "%s differs: %u there, %u here", name_of(i), theirs[i], ours[i]);
      return buf;
    }
  if (n_theirs != ours.size()) {
    snprintf(buf, sizeof buf, "signature length differs: %zu words there, %zu here", n_theirs, ours.size());
    return buf;
  }
  return std::string();
}

size_t slot_bytes_of(const SlotXfer& x, bool with_opt) { return x.bytes_base + (with_opt ? x.bytes_opt : 0); }

bool slot_xfer_fits(const SlotXfer& x, int n, bool host, bool with_opt) {
  const size_t need = (size_t)n * slot_bytes_of(x, with_opt);
  return x.d_secs && x.ev_packed && (!with_opt || x.d_has_opt) && n <= x.slots_cap && need <= x.d_stage_cap && (!host || need <= x.h_stage_cap);
}

// Device side of the table and the staging buffers, sized for n slots.  has_opt: the optional group exists; `opt` holds its
// sections (for their bases) when the device table does not have them yet.  Called with SlotXfer::mu and the API lock's
// exclusive side held.
int slot_stage_ensure(DsmDevice* e, SlotXfer& x, int n, bool host, bool has_opt, const std::vector<SlotSection>& opt) {
  if (slot_xfer_fits(x, n, host, has_opt)) return 0;
  if (!x.ev_packed)
    if (int rc = e->new_event(&x.ev_packed)) return rc;
  if (!x.d_secs)
    if (int rc = e->dalloc(&x.d_secs, x.secs.size())) return rc;
  if (!x.d_has_opt) {  // first time, or the optional group came into being since
    if (has_opt)
      for (int i = 0; i < x.nsec_opt; ++i) x.secs[(size_t)x.nsec_base + i].base = opt[(size_t)i].base;
    HIPCHK(hipMemcpy(x.d_secs, x.secs.data(), sizeof(SlotSection) * x.secs.size(), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    x.d_has_opt = has_opt;
  }
  if (n > x.slots_cap) {
    e->dfree(x.d_slots);
    x.d_slots = nullptr;
    x.slots_cap = 0;
    if (int rc = e->dalloc(&x.d_slots, (size_t)n)) return rc;
    x.slots_cap = n;
  }
  const size_t need = (size_t)n * slot_bytes_of(x, has_opt);
  if (need > x.d_stage_cap) {
    e->dfree(x.d_stage);
    x.d_stage = nullptr;
    x.d_stage_cap = 0;
    if (int rc = e->dalloc(&x.d_stage, need, false)) return rc;
    x.d_stage_cap = need;
  }
  if (host && need > x.h_stage_cap) {
    e->hfree(x.h_stage);
    x.h_stage = nullptr;
    x.h_stage_cap = 0;
    if (int rc = e->halloc(&x.h_stage, need)) return rc;
    x.h_stage_cap = need;
  }
  return 0;
}

// One launch: the n slots listed at d_slots <-> stage, slot j at stage + j * slot_bytes.  Tables and slot list are x's; the
// staging buffer may be another engine's (move).  with_opt: the optional group's sections too.
int slot_launch(DsmDevice* e, const SlotXfer& x, hipStream_t st, bool pack, int n, bool with_opt, char* stage) {
  const int nsec = x.nsec_base + (with_opt ? x.nsec_opt : 0);
  const unsigned chunks = x.chunks_base + (with_opt ? x.chunks_opt : 0);
  const long slot_bytes = (long)slot_bytes_of(x, with_opt);
  // a couple of thousand workgroups in all (eight per CU); each strides over the pieces that are left
  unsigned gx = 2048u / (unsigned)n;
  if (gx < 1) gx = 1;
  if (gx > chunks) gx = chunks;
  if (pack)
    hipLaunchKernelGGL(slot_state_pack_kernel, dim3(gx, (unsigned)n), dim3(256), 0, st, (const SlotSection*)x.d_secs, nsec, chunks,
                       (const int*)x.d_slots, stage, slot_bytes);
  else
    hipLaunchKernelGGL(slot_state_unpack_kernel, dim3(gx, (unsigned)n), dim3(256), 0, st, (const SlotSection*)x.d_secs, nsec, chunks,
                       (const int*)x.d_slots, stage, slot_bytes);
  HIPCHK(hipGetLastError());
  return 0;
}

// The gaps behind sections that are no multiple of 16 are not written by the pack kernel: defined bytes in a blob's payload.
void slot_zero_gaps(const SlotXfer& x, uint8_t* payload, int n, bool with_opt) {
  const int nsec = x.nsec_base + (with_opt ? x.nsec_opt : 0);
  const size_t sb = slot_bytes_of(x, with_opt);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < nsec; ++s) {
      const SlotSection& sec = x.secs[(size_t)s];
      const size_t gap = (size_t)dsm_blob::align16((uint64_t)sec.bytes) - (size_t)sec.bytes;
      if (gap) memset(payload + (size_t)i * sb + (size_t)sec.off + (size_t)sec.bytes, 0, gap);
    }
}

// A caller's slot list against an engine of B slots.
int slot_check_list(DsmDevice* e, int B, const int* slots, int n, bool distinct, const char* what) {
  if (!slots || n < 1) { e->set_error("%s: empty slot list", what); return DSM_ERR_INVALID; }
  if (n > B) { e->set_error("%s: %d slots listed, the engine has %d", what, n, B); return DSM_ERR_INVALID; }
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= B) {
      e->set_error("%s: batch index out of range: %d >= %d", what, slots[i], B);
      return DSM_ERR_INVALID;
    }
  if (distinct) {
    std::vector<uint8_t> seen((size_t)B, 0);
    for (int i = 0; i < n; ++i) {
      if (seen[(size_t)slots[i]]) { e->set_error("%s: slot %d is listed twice", what, slots[i]); return DSM_ERR_INVALID; }
      seen[(size_t)slots[i]] = 1;
    }
  }
  return 0;
}

}  // namespace
