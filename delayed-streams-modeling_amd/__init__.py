"""dsm_amd — Python binding of libdsm_mi355x.so (the C ABI in include/dsm.h).

This is plumbing for tests / bench / smoke: ctypes mirrors of the config structs and thin
wrappers that hand numpy (host) or torch (device) buffers to the C entry points.  The compute
lives in the HIP library; there is NO Python or CPU fallback — if the library or the GPU is
missing, calls raise.

The directory name carries a hyphen (it mirrors the upstream repo name), so import it through
the `dsm_amd` shim at the repo root.
"""
import collections
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdsm_mi355x.so")

FRAME_SIZE = 1920
MAX_RATIOS = 8
MAX_EXTRA_HEADS = 8


class TransformerConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "d_model", "num_heads", "num_layers", "dim_feedforward", "context", "max_period",
        "gating", "norm", "positional_embedding", "layer_scale", "conv_layout")]


class MimiConfig(C.Structure):
    _fields_ = [
        ("channels", C.c_int), ("dimension", C.c_int), ("n_filters", C.c_int),
        ("n_residual_layers", C.c_int), ("n_ratios", C.c_int), ("ratios", C.c_int * MAX_RATIOS),
        ("kernel_size", C.c_int), ("residual_kernel_size", C.c_int), ("last_kernel_size", C.c_int),
        ("dilation_base", C.c_int), ("compress", C.c_int), ("transformer", TransformerConfig),
        ("quantizer_n_q", C.c_int), ("quantizer_bins", C.c_int), ("quantizer_dim", C.c_int),
        ("downsample_stride", C.c_int)]


class AsrConfig(C.Structure):
    _fields_ = [
        ("lm", TransformerConfig), ("text_in_vocab_size", C.c_int), ("text_out_vocab_size", C.c_int),
        ("audio_vocab_size", C.c_int), ("audio_codebooks", C.c_int), ("extra_heads_num", C.c_int),
        ("extra_heads_dim", C.c_int), ("asr_delay_in_tokens", C.c_int), ("temperature", C.c_float),
        ("mimi", MimiConfig), ("kv_bf16", C.c_int), ("dot_mode", C.c_int)]

    def copy(self):
        out = AsrConfig()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(AsrConfig))
        return out


class TtsConfig(C.Structure):
    """dsm_tts_config (include/dsm.h): lm::Config + DepFormerConfig + tts_streaming::Config."""
    _fields_ = [
        ("lm", TransformerConfig), ("text_in_vocab_size", C.c_int), ("text_out_vocab_size", C.c_int),
        ("audio_vocab_size", C.c_int), ("audio_codebooks", C.c_int), ("depformer", TransformerConfig),
        ("dep_num_slices", C.c_int), ("dep_low_rank", C.c_int), ("dep_weight_groups", C.c_int),
        ("acoustic_delay", C.c_int), ("text_pad_token", C.c_int), ("text_bos_token", C.c_int),
        ("text_eos_token", C.c_int), ("text_eop_token", C.c_int), ("text_start_token", C.c_int),
        ("text_audio_delay_in_tokens", C.c_int), ("max_consecutive_pads", C.c_int), ("max_steps", C.c_int),
        ("kv_bf16", C.c_int), ("cross_attention", C.c_int), ("ca_norm", C.c_int), ("ca_dim", C.c_int),
        ("ca_max_len", C.c_int), ("cfg_rows", C.c_int), ("dot_mode", C.c_int)]


TTS_UNGENERATED = 0xFFFFFFFF
TTS_ALLOW_PAD, TTS_ALLOW_PAD_OR_EPAD = -1, -2


class InMsg(C.Structure):
    _fields_ = [("kind", C.c_int), ("id", C.c_int64), ("pcm", C.c_void_p), ("n_pcm", C.c_size_t),
                ("data", C.c_void_p), ("n_data", C.c_size_t)]


class OutMsg(C.Structure):
    _fields_ = [("kind", C.c_int), ("text", C.c_char_p), ("time", C.c_double), ("id", C.c_int64),
                ("step_idx", C.c_uint64), ("prs", C.c_void_p), ("n_prs", C.c_size_t), ("buffered_pcm", C.c_uint64)]


IN_KINDS = ["Init", "Marker", "Audio", "OggOpus", "Ping"]
OUT_KINDS = ["Word", "EndWord", "Marker", "Step", "Error", "Ready"]
DETOK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_size_t)


class AsrMsg(C.Structure):
    _fields_ = [("kind", C.c_int), ("batch_idx", C.c_int), ("step_idx", C.c_int), ("time", C.c_double),
                ("tokens_offset", C.c_int), ("n_tokens", C.c_int), ("prs", C.c_float * MAX_EXTRA_HEADS)]


BE_ENCODE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8))
BE_RESET = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
BE_STEP = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float))
BE_POLL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(AsrMsg), C.c_int, C.POINTER(C.c_uint32), C.c_int)
BE_ERROR = C.CFUNCTYPE(C.c_char_p, C.c_void_p)
BE_ENCODE_ASYNC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int))
BE_STEP_TICKET = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float))


class WorkerBackend(C.Structure):
    """dsm_worker_backend (include/dsm.h)."""
    _fields_ = [("self", C.c_void_p), ("batch_size", C.c_int), ("asr_delay_in_tokens", C.c_int),
                ("extra_heads_num", C.c_int), ("encode_step", BE_ENCODE), ("reset_slot", BE_RESET),
                ("step_tokens", BE_STEP), ("poll_msgs", BE_POLL), ("last_error", BE_ERROR),
                ("encode_async", BE_ENCODE_ASYNC), ("step_ticket", BE_STEP_TICKET), ("text_out_vocab_size", C.c_int)]


class Metrics(C.Structure):
    _fields_ = [("last_encode_us", C.c_double), ("last_lm_us", C.c_double),
                ("algorithmic_bytes_encode", C.c_double), ("algorithmic_bytes_lm", C.c_double),
                ("steps_encode", C.c_uint64), ("steps_lm", C.c_uint64),
                ("graph_launches", C.c_uint64), ("eager_bodies", C.c_uint64),
                ("capture_failures", C.c_uint64), ("capture_error", C.c_char * 96)]


class SlotBlobInfo(C.Structure):
    _fields_ = [("version", C.c_uint32), ("n_slots", C.c_uint32), ("flags", C.c_uint32), ("sig_words", C.c_uint32),
                ("host_bytes", C.c_uint64), ("slot_bytes", C.c_uint64), ("total_bytes", C.c_uint64)]


class TtsSlotBlobInfo(C.Structure):
    _fields_ = [("version", C.c_uint32), ("n_slots", C.c_uint32), ("flags", C.c_uint32), ("sig_words", C.c_uint32),
                ("slices", C.c_uint32), ("reserved", C.c_uint32),
                ("host_bytes", C.c_uint64), ("slot_bytes", C.c_uint64), ("total_bytes", C.c_uint64)]


SLOT_BLOB_HAS_MODEL_MIMI = 1
TTS_SLOT_BLOB_HAS_MIMI_DEC = 1
MSG_STEP, MSG_WORD, MSG_END_WORD = 0, 1, 2

# Every symbol include/dsm.h declares (the "not gpu" tests check the library exports all of them).
ABI_SYMBOLS = [
    "dsm_mimi_config_v0_1", "dsm_asr_config_stt_1b_en_fr", "dsm_asr_config_stt_2_6b_en",
    "dsm_asr_create", "dsm_asr_create_from_arena", "dsm_asr_weight_arena", "dsm_destroy", "dsm_last_error", "dsm_mimi_encode_step", "dsm_asr_step_tokens",
    "dsm_asr_step_pcm", "dsm_asr_poll_msgs", "dsm_asr_reset_slot", "dsm_mimi_reset_slot", "dsm_sync",
    "dsm_get_metrics", "dsm_batch_size", "dsm_n_q", "dsm_mimi_encode_step_dev", "dsm_asr_step_tokens_dev",
    "dsm_streams_join", "dsm_debug_read", "dsm_debug_gemm_plan", "dsm_debug_gemm_plan_knobs", "dsm_debug_gemm", "dsm_asr_step_pcm_dev", "dsm_prof_enable", "dsm_prof_read",
    "dsm_asr_export_slots", "dsm_asr_import_slots", "dsm_asr_move_slots", "dsm_slot_blob_info",
    "dsm_asr_create_replica", "dsm_asr_set_seed", "dsm_debug_set_positions", "dsm_debug_set_text_tokens", "dsm_mimi_decode_step", "dsm_mimi_decode_step_dev",
    "dsm_lm_stream_groups", "dsm_debug_serialize_groups", "dsm_prof_read_device", "dsm_prof_timeline", "dsm_prof_timeline_read",
    "dsm_wav_decode", "dsm_mp3_decode", "dsm_mp3_decode_info", "dsm_mp3_probe", "dsm_resample", "dsm_pcm_decode",
    "dsm_mp3_test_synth", "dsm_mp3_test_tables", "dsm_mp3_test_imdct", "dsm_free", "dsm_linear_resampler_new", "dsm_linear_resampler_process",
    "dsm_linear_resampler_free", "dsm_ogg_demux_new", "dsm_ogg_demux_free", "dsm_ogg_demux_push", "dsm_ogg_demux_next",
    "dsm_ogg_demux_info", "dsm_worker_set_opus_decoder", "dsm_ogg_mux_new", "dsm_ogg_mux_free", "dsm_ogg_mux_header", "dsm_ogg_mux_page",
    "dsm_inmsg_encode", "dsm_outmsg_encode", "dsm_inmsg_decode", "dsm_outmsg_decode", "dsm_worker_create",
    "dsm_worker_create_with_backend", "dsm_worker_destroy", "dsm_worker_last_error", "dsm_worker_set_detokenizer", "dsm_worker_open", "dsm_worker_close",
    "dsm_worker_send", "dsm_worker_send_body", "dsm_worker_step", "dsm_worker_step_encode", "dsm_worker_step_model",
    "dsm_mimi_encode_step_async", "dsm_asr_step_tokens_ticket", "dsm_worker_recv", "dsm_worker_buffered",
    "dsm_tts_config_v202501", "dsm_tts_create", "dsm_tts_destroy", "dsm_tts_last_error", "dsm_tts_step",
    "dsm_tts_audio_tokens", "dsm_tts_step_idx", "dsm_tts_reset_slot", "dsm_tts_debug_read", "dsm_tts_get_metrics", "dsm_tts_set_sampling",
    "dsm_tts_set_ca_src", "dsm_tts_attach_mimi", "dsm_tts_step_pcm", "dsm_tts_recv_pcm", "dsm_tts_pcm_pending",
    "dsm_tts_attach_speaker_encoder", "dsm_tts_encode_voice", "dsm_tts_speaker_empty",
    "dsm_tts_voice_create", "dsm_tts_voice_destroy", "dsm_tts_voice_info", "dsm_tts_set_voice",
    "dsm_tts_request_begin", "dsm_tts_request_push_words", "dsm_tts_request_close", "dsm_tts_run", "dsm_tts_collect",
    "dsm_tts_request_status",
    "dsm_tts_attach_conditioners", "dsm_tts_set_condition_lut", "dsm_tts_set_condition_cont", "dsm_tts_set_condition_padding",
    "dsm_tts_clear_condition",
    "dsm_spm_load", "dsm_spm_load_bytes", "dsm_spm_free", "dsm_spm_last_error", "dsm_spm_vocab_size", "dsm_spm_special_ids",
    "dsm_spm_encode", "dsm_spm_decode", "dsm_worker_set_tokenizer_file",
    "dsm_tts_attach_tokenizer", "dsm_tts_request_push_text", "dsm_tts_word_text",
    "dsm_tts_slot_blob_info", "dsm_tts_slot_layout",
    "dsm_asr_set_token_scores", "dsm_asr_token_scores", "dsm_asr_token_scores_dev", "dsm_asr_poll_word_scores",
    "dsm_token_scores_host", "dsm_debug_token_scores", "dsm_worker_set_word_scores",
    "dsm_asr_set_text_bias", "dsm_asr_bias_create", "dsm_asr_bias_create_text", "dsm_asr_bias_destroy", "dsm_asr_bias_info",
    "dsm_asr_set_bias", "dsm_asr_bias_state", "dsm_text_bias_compile", "dsm_text_bias_pick_host", "dsm_debug_text_pick",
    "dsm_worker_set_bias",
    "dsm_asr_set_ingest", "dsm_asr_set_input_format", "dsm_asr_input_format", "dsm_mimi_encode_step_raw",
    "dsm_mimi_encode_step_raw_async", "dsm_mimi_encode_step_raw_dev", "dsm_asr_step_raw", "dsm_debug_ingest_read",
    "dsm_ingest_host_new", "dsm_ingest_host_free", "dsm_ingest_host", "dsm_ingest_describe", "dsm_ingest_g711_table",
    "dsm_worker_set_input_rate",
    "dsm_tts_set_egress", "dsm_tts_set_output_format", "dsm_tts_output_format", "dsm_tts_step_raw", "dsm_tts_recv_raw",
    "dsm_tts_collect_raw", "dsm_tts_debug_egress", "dsm_egress_host_new", "dsm_egress_host_free", "dsm_egress_host",
    "dsm_egress_describe", "dsm_egress_encode_sample",
    "dsm_asr_set_clips", "dsm_asr_clip_begin", "dsm_asr_clip_push", "dsm_asr_clip_close", "dsm_asr_run", "dsm_asr_collect",
    "dsm_asr_clip_status", "dsm_asr_clip_frame_host", "dsm_asr_clip_host_new", "dsm_asr_clip_host_free", "dsm_asr_clip_host_begin",
    "dsm_asr_clip_host_push", "dsm_asr_clip_host_close", "dsm_asr_clip_host_reset", "dsm_asr_clip_host_status", "dsm_asr_clip_host_run",
]
PCM_F32, PCM_S16, PCM_MULAW, PCM_ALAW = 0, 1, 2, 3  # DSM_PCM_*: the sample formats of the ingest and egress sections
INGEST_MAX_FRAME_BYTES = 15360  # the largest raw frame (48 kHz f32) and the largest pitch of the raw calls
EGRESS_MAX_FRAME_BYTES = 15360  # the same on the way out: the largest row and pitch of the TTS raw calls
BIAS_MAX_TOKENS, BIAS_MAX_KEYWORD_TOKENS, BIAS_MAX_NODES, BIAS_MAX_SETS = 1024, 32, 65535, 256  # DSM_BIAS_MAX_*
BIAS_DEAD = 0xFFFFFFFF  # DSM_BIAS_DEAD: the trie node of a slot inside a word that left the trie


class DebugRowMap(C.Structure):
    """dsm_debug_rowmap (include/dsm.h): row r starts at element (r // rpb) * bstride + (r % rpb + toff) * ld."""
    _fields_ = [("bstride", C.c_int64), ("rpb", C.c_int32), ("ld", C.c_int32), ("toff", C.c_int32), ("pad_", C.c_int32)]


class DebugGemmArgs(C.Structure):
    """dsm_debug_gemm_args (include/dsm.h)."""
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("weight_bf16", C.c_int32), ("epi", C.c_int32), ("act", C.c_int32), ("may_defer", C.c_int32), ("norm_rms", C.c_int32),
                ("knobs", C.c_int32 * 5), ("w_changed", C.c_int32),
                ("X", C.c_void_p), ("x_len", C.c_uint64), ("xmap", DebugRowMap),
                ("W", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p),
                ("res", C.c_void_p), ("res_len", C.c_uint64), ("rmap", DebugRowMap),
                ("Y", C.c_void_p), ("y_len", C.c_uint64), ("ymap", DebugRowMap),
                ("Y2", C.c_void_p), ("y2_len", C.c_uint64), ("y2map", DebugRowMap),
                ("norm_w", C.c_void_p), ("norm_b", C.c_void_p), ("norm_out", C.c_void_p), ("norm_len", C.c_uint64),
                ("x_back", C.c_void_p), ("res_back", C.c_void_p)]


EPI_STORE, EPI_QKV, EPI_GATE, EPI_RVQ = 0, 1, 2, 3  # the GEMM epilogues (dsm_debug_gemm_plan, dsm_debug_gemm)


class BiasToken(C.Structure):
    """dsm_bias_token (include/dsm.h)."""
    _fields_ = [("token", C.c_uint32), ("bias", C.c_float)]


class BiasKeyword(C.Structure):
    """dsm_bias_keyword (include/dsm.h): one word as its piece ids, and its boost in logit units."""
    _fields_ = [("tokens", C.POINTER(C.c_uint32)), ("n_tokens", C.c_int), ("boost", C.c_float)]


SCORES_MAX_TOP = 8  # DSM_SCORES_MAX_TOP
SCORES_NONE = 0xFFFFFFFF  # the id of a top-N entry beyond the vocabulary
TTS_COND_LUT, TTS_COND_CONTINUOUS = 0, 1  # DSM_TTS_COND_*
TTS_RUN_MAX = 16  # DSM_TTS_RUN_MAX
TTS_REQ_IDLE, TTS_REQ_RUNNING, TTS_REQ_WAITING, TTS_REQ_DONE, TTS_REQ_DONE_LIMIT = range(5)  # DSM_TTS_REQ_*


class TtsWordEvent(C.Structure):
    """dsm_tts_word_event: steps, not seconds (divide by 12.5, srv/tts.rs:599-600); word -1 is the initial empty word."""
    _fields_ = [("slot", C.c_int), ("word", C.c_int), ("start_step", C.c_int), ("stop_step", C.c_int)]


class TtsBlockC(C.Structure):
    """dsm_tts_block (include/dsm.h): caller-provided arrays of one dsm_tts_run block."""
    _fields_ = [("n_steps", C.c_int), ("stepped", C.c_void_p), ("text_token", C.c_void_p), ("audio", C.c_void_p),
                ("pcm", C.c_void_p), ("pcm_valid", C.c_void_p), ("events", C.POINTER(TtsWordEvent)),
                ("events_cap", C.c_int), ("n_events", C.c_int), ("status", C.c_void_p)]


class TtsConditionerDesc(C.Structure):
    """dsm_tts_conditioner_desc (include/dsm.h): one entry of [modules.<m>.model.conditioners]."""
    _fields_ = [("name", C.c_char_p), ("type", C.c_int), ("dim", C.c_int), ("n_bins", C.c_int),
                ("possible_values", C.POINTER(C.c_char_p)), ("n_values", C.c_int),
                ("scale_factor", C.c_float), ("max_period", C.c_float)]


ASR_RUN_MAX = 16  # DSM_ASR_RUN_MAX
ASR_CLIP_IDLE, ASR_CLIP_RUNNING, ASR_CLIP_WAITING, ASR_CLIP_DONE = range(4)  # DSM_ASR_CLIP_*


class AsrBlockC(C.Structure):
    """dsm_asr_block (include/dsm.h): caller-provided arrays of one dsm_asr_run block."""
    _fields_ = [("n_steps", C.c_int), ("stepped", C.c_void_p), ("text_token", C.c_void_p), ("vad_prs", C.c_void_p),
                ("logprob", C.c_void_p), ("msgs", C.POINTER(AsrMsg)), ("msg_step", C.POINTER(C.c_int)), ("msgs_cap", C.c_int),
                ("n_msgs", C.c_int), ("msg_tokens", C.c_void_p), ("msg_logprobs", C.c_void_p), ("tokens_cap", C.c_int),
                ("n_tokens", C.c_int), ("status", C.c_void_p)]


AsrBlock = collections.namedtuple("AsrBlock", "n_steps stepped text_token vad_prs logprob msgs word_scores status")
TtsBlock = collections.namedtuple("TtsBlock", "n_steps stepped text_token audio pcm pcm_valid events status")
PROF_TAGS = ["attn_lm", "gemm_lm", "attn_mimi", "gemm_mimi", "rvq", "other"]

_lib = None


def load_library(path=None):
    """dlopen the HIP library (no GPU needed for this) and declare signatures."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no CPU fallback for the MI355X engine.")
    lib = C.CDLL(p)
    vp, ip, u8p, u32p, fp = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p
    lib.dsm_mimi_config_v0_1.argtypes = [C.POINTER(MimiConfig), C.c_int]
    lib.dsm_asr_config_stt_1b_en_fr.argtypes = [C.POINTER(AsrConfig)]
    lib.dsm_asr_config_stt_2_6b_en.argtypes = [C.POINTER(AsrConfig)]
    lib.dsm_asr_create.argtypes = [C.POINTER(AsrConfig), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(vp)]
    lib.dsm_asr_create.restype = C.c_int
    lib.dsm_asr_create_from_arena.argtypes = [C.POINTER(AsrConfig), C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
    lib.dsm_asr_weight_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.dsm_destroy.argtypes = [vp]
    lib.dsm_destroy.restype = None
    lib.dsm_last_error.argtypes = [vp]
    lib.dsm_last_error.restype = C.c_char_p
    lib.dsm_mimi_encode_step.argtypes = [vp, fp, u8p, u32p, C.POINTER(C.c_int)]
    lib.dsm_asr_step_tokens.argtypes = [vp, u32p, u8p, u32p, fp]
    lib.dsm_asr_step_pcm.argtypes = [vp, fp, u8p, u32p, u32p, fp]
    lib.dsm_asr_poll_msgs.argtypes = [vp, C.POINTER(AsrMsg), C.c_int, u32p, C.c_int]
    lib.dsm_asr_reset_slot.argtypes = [vp, C.c_int]
    lib.dsm_mimi_reset_slot.argtypes = [vp, C.c_int]
    lib.dsm_sync.argtypes = [vp]
    lib.dsm_get_metrics.argtypes = [vp, C.POINTER(Metrics)]
    lib.dsm_batch_size.argtypes = [vp]
    lib.dsm_n_q.argtypes = [vp]
    lib.dsm_mimi_encode_step_dev.argtypes = [vp, vp, vp, vp]
    lib.dsm_asr_step_tokens_dev.argtypes = [vp, vp, vp, vp, vp]
    lib.dsm_streams_join.argtypes = [vp]
    lib.dsm_debug_read.argtypes = [vp, C.c_char_p, fp, C.c_size_t]
    lib.dsm_asr_step_pcm_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dsm_mimi_decode_step.argtypes = [vp, u32p, u8p, fp, C.POINTER(C.c_int)]
    lib.dsm_mimi_decode_step.restype = C.c_int
    lib.dsm_mimi_decode_step_dev.argtypes = [vp, vp, vp, vp]
    lib.dsm_mimi_decode_step_dev.restype = C.c_int
    lib.dsm_debug_set_positions.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.dsm_debug_set_positions.restype = C.c_int
    lib.dsm_asr_create_replica.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.dsm_asr_create_replica.restype = C.c_int
    lib.dsm_asr_set_seed.argtypes = [vp, C.c_int, C.c_uint64]
    lib.dsm_asr_set_seed.restype = C.c_int
    lib.dsm_debug_set_text_tokens.argtypes = [vp, vp]
    lib.dsm_asr_export_slots.argtypes = [vp, C.POINTER(C.c_int), C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dsm_asr_import_slots.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_size_t]
    lib.dsm_asr_move_slots.argtypes = [vp, C.POINTER(C.c_int), vp, C.POINTER(C.c_int), C.c_int]
    lib.dsm_slot_blob_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(SlotBlobInfo)]
    lib.dsm_mimi_encode_step_async.argtypes = [vp, fp, u8p, C.POINTER(C.c_int)]
    lib.dsm_asr_step_tokens_ticket.argtypes = [vp, C.c_int, u8p, u32p, fp]
    for name in ("dsm_asr_export_slots", "dsm_asr_import_slots", "dsm_asr_move_slots", "dsm_slot_blob_info"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_debug_set_text_tokens.restype = C.c_int
    lib.dsm_prof_enable.argtypes = [vp, C.c_uint]
    lib.dsm_prof_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    for name in ("dsm_mimi_encode_step", "dsm_asr_step_tokens", "dsm_asr_step_pcm", "dsm_asr_poll_msgs",
                 "dsm_asr_reset_slot", "dsm_mimi_reset_slot", "dsm_sync", "dsm_get_metrics", "dsm_batch_size",
                 "dsm_n_q", "dsm_mimi_encode_step_dev", "dsm_asr_step_tokens_dev", "dsm_streams_join",
                 "dsm_debug_read", "dsm_asr_step_pcm_dev", "dsm_prof_enable", "dsm_prof_read"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_prof_read_device.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.dsm_prof_read_device.restype = C.c_int
    lib.dsm_lm_stream_groups.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.dsm_lm_stream_groups.restype = C.c_int
    lib.dsm_debug_serialize_groups.argtypes = [vp, C.c_int]
    lib.dsm_debug_serialize_groups.restype = C.c_int
    lib.dsm_debug_gemm_plan.argtypes = [C.c_int] * 9 + [C.c_char_p, C.c_size_t]
    lib.dsm_debug_gemm_plan.restype = C.c_int
    lib.dsm_debug_gemm_plan_knobs.argtypes = [C.c_int, C.POINTER(C.c_int)] + [C.c_int] * 7 + [C.c_char_p, C.c_size_t]
    lib.dsm_debug_gemm_plan_knobs.restype = C.c_int
    lib.dsm_debug_gemm.argtypes = [vp, C.POINTER(DebugGemmArgs), C.c_char_p, C.c_size_t]
    lib.dsm_debug_gemm.restype = C.c_int
    lib.dsm_wav_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_int)]
    lib.dsm_wav_decode.restype = C.c_int
    for name in ("dsm_mp3_decode", "dsm_pcm_decode"):
        getattr(lib, name).argtypes = lib.dsm_wav_decode.argtypes
        getattr(lib, name).restype = C.c_int
    lib.dsm_mp3_decode_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t), C.POINTER(Mp3Info)]
    lib.dsm_mp3_decode_info.restype = C.c_int
    lib.dsm_mp3_probe.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Mp3Info)]
    lib.dsm_mp3_probe.restype = C.c_int
    lib.dsm_resample.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t)]
    lib.dsm_resample.restype = C.c_int
    lib.dsm_mp3_test_synth.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.dsm_mp3_test_tables.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
    lib.dsm_mp3_test_imdct.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.dsm_free.argtypes = [vp]
    lib.dsm_free.restype = None
    lib.dsm_linear_resampler_new.argtypes = [C.c_uint32, C.c_uint32]
    lib.dsm_linear_resampler_new.restype = vp
    lib.dsm_linear_resampler_process.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    lib.dsm_linear_resampler_process.restype = C.c_size_t
    lib.dsm_linear_resampler_free.argtypes = [vp]
    lib.dsm_linear_resampler_free.restype = None
    lib.dsm_inmsg_encode.argtypes = [C.POINTER(InMsg), vp, C.c_size_t]
    lib.dsm_outmsg_encode.argtypes = [C.POINTER(OutMsg), vp, C.c_size_t]
    lib.dsm_inmsg_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(InMsg), vp, C.c_size_t, vp, C.c_size_t]
    lib.dsm_outmsg_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OutMsg), vp, C.c_size_t, vp, C.c_size_t]
    lib.dsm_worker_create.argtypes = [vp, C.POINTER(vp)]
    lib.dsm_worker_create_with_backend.argtypes = [C.POINTER(WorkerBackend), C.POINTER(vp)]
    lib.dsm_worker_create_with_backend.restype = C.c_int
    lib.dsm_worker_destroy.argtypes = [vp]
    lib.dsm_worker_destroy.restype = None
    lib.dsm_worker_last_error.argtypes = [vp]
    lib.dsm_worker_last_error.restype = C.c_char_p
    lib.dsm_worker_set_detokenizer.argtypes = [vp, DETOK_FN, vp]
    lib.dsm_worker_set_detokenizer.restype = None
    lib.dsm_worker_open.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.dsm_worker_close.argtypes = [vp, C.c_int]
    lib.dsm_worker_send.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    lib.dsm_worker_step.argtypes = [vp]
    lib.dsm_worker_step_encode.argtypes = [vp]
    lib.dsm_worker_step_model.argtypes = [vp]
    lib.dsm_worker_recv.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dsm_worker_buffered.argtypes = [vp, C.c_int]
    for name in ("dsm_inmsg_encode", "dsm_outmsg_encode", "dsm_inmsg_decode", "dsm_outmsg_decode", "dsm_worker_create",
                 "dsm_worker_open", "dsm_worker_close", "dsm_worker_send", "dsm_worker_step", "dsm_worker_step_encode", "dsm_worker_step_model",
    "dsm_mimi_encode_step_async", "dsm_asr_step_tokens_ticket", "dsm_worker_recv",
                 "dsm_worker_buffered"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_tts_config_v202501.argtypes = [C.POINTER(TtsConfig)]
    lib.dsm_tts_config_v202501.restype = None
    lib.dsm_tts_create.argtypes = [C.POINTER(TtsConfig), C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]
    lib.dsm_tts_destroy.argtypes = [vp]
    lib.dsm_tts_destroy.restype = None
    lib.dsm_tts_last_error.argtypes = [vp]
    lib.dsm_tts_last_error.restype = C.c_char_p
    lib.dsm_tts_step.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dsm_tts_audio_tokens.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.dsm_tts_step_idx.argtypes = [vp, C.c_int]
    lib.dsm_tts_reset_slot.argtypes = [vp, C.c_int]
    lib.dsm_tts_debug_read.argtypes = [vp, C.c_char_p, fp, C.c_size_t]
    lib.dsm_tts_get_metrics.argtypes = [vp, C.POINTER(Metrics)]
    lib.dsm_tts_set_sampling.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_uint64]
    lib.dsm_tts_set_ca_src.argtypes = [vp, C.c_int, fp, C.c_int, fp, C.c_int, C.c_double]
    lib.dsm_tts_attach_mimi.argtypes = [vp, C.POINTER(MimiConfig), C.c_char_p]
    lib.dsm_tts_step_pcm.argtypes = [vp, vp, vp, vp, vp, vp, fp, u8p]
    lib.dsm_tts_recv_pcm.argtypes = [vp, fp, u8p]
    lib.dsm_tts_pcm_pending.argtypes = [vp]
    lib.dsm_tts_attach_speaker_encoder.argtypes = [vp, C.c_int, C.c_char_p]
    lib.dsm_tts_voice_create.argtypes = [vp, fp, C.c_int, C.POINTER(C.c_int)]
    lib.dsm_tts_voice_destroy.argtypes = [vp, C.c_int]
    lib.dsm_tts_voice_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    lib.dsm_tts_set_voice.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.dsm_tts_encode_voice.argtypes = [vp, fp, C.c_int, C.c_int, fp, C.c_int, C.POINTER(C.c_int)]
    lib.dsm_tts_speaker_empty.argtypes = [vp, fp, C.c_int, C.POINTER(C.c_int)]
    lib.dsm_tts_request_begin.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.dsm_tts_request_push_words.argtypes = [vp, C.c_int, u32p, vp, C.c_int]
    lib.dsm_tts_request_close.argtypes = [vp, C.c_int]
    lib.dsm_tts_run.argtypes = [vp, C.c_int, C.c_int]
    lib.dsm_tts_collect.argtypes = [vp, C.POINTER(TtsBlockC)]
    lib.dsm_tts_request_status.argtypes = [vp, C.c_int]
    lib.dsm_tts_attach_conditioners.argtypes = [vp, C.POINTER(TtsConditionerDesc), C.c_int, C.c_char_p]
    lib.dsm_tts_set_condition_lut.argtypes = [vp, C.c_int, C.c_char_p, C.c_char_p]
    lib.dsm_tts_set_condition_cont.argtypes = [vp, C.c_int, C.c_char_p, C.c_float]
    lib.dsm_tts_set_condition_padding.argtypes = [vp, C.c_int, C.c_char_p]
    lib.dsm_tts_clear_condition.argtypes = [vp, C.c_int]
    lib.dsm_spm_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.dsm_spm_load_bytes.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    lib.dsm_spm_free.argtypes = [vp]
    lib.dsm_spm_free.restype = None
    lib.dsm_spm_last_error.argtypes = [vp]
    lib.dsm_spm_last_error.restype = C.c_char_p
    lib.dsm_spm_vocab_size.argtypes = [vp]
    lib.dsm_spm_special_ids.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    lib.dsm_spm_encode.argtypes = [vp, C.c_char_p, C.c_size_t, u32p, C.c_size_t]
    lib.dsm_spm_encode.restype = C.c_int64
    lib.dsm_spm_decode.argtypes = [vp, u32p, C.c_size_t, vp, C.c_size_t]
    lib.dsm_spm_decode.restype = C.c_int64
    lib.dsm_worker_set_tokenizer_file.argtypes = [vp, C.c_char_p]
    lib.dsm_tts_attach_tokenizer.argtypes = [vp, C.c_char_p]
    lib.dsm_tts_request_push_text.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    lib.dsm_tts_word_text.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    lib.dsm_tts_word_text.restype = C.c_int64
    lib.dsm_tts_slot_blob_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(TtsSlotBlobInfo)]
    lib.dsm_tts_slot_blob_info.restype = C.c_int
    lib.dsm_tts_slot_layout.argtypes = [C.POINTER(TtsConfig), C.POINTER(MimiConfig), C.c_char_p, C.c_size_t]
    lib.dsm_tts_slot_layout.restype = C.c_int
    lib.dsm_asr_set_token_scores.argtypes = [vp, C.c_int]
    lib.dsm_asr_token_scores.argtypes = [vp, fp, u32p, fp]
    lib.dsm_asr_token_scores_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.dsm_asr_poll_word_scores.argtypes = [vp, fp, C.c_int]
    lib.dsm_token_scores_host.argtypes = [fp, C.c_int, C.c_uint32, C.c_int, fp, u32p, fp]
    lib.dsm_debug_token_scores.argtypes = [vp, fp, C.c_int, C.c_int, u32p, C.c_int, fp, u32p, fp]
    lib.dsm_worker_set_word_scores.argtypes = [vp, C.c_int]
    for name in ("dsm_asr_set_token_scores", "dsm_asr_token_scores", "dsm_asr_token_scores_dev", "dsm_asr_poll_word_scores",
                 "dsm_token_scores_host", "dsm_debug_token_scores", "dsm_worker_set_word_scores"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_asr_set_text_bias.argtypes = [vp, C.c_int]
    lib.dsm_asr_bias_create.argtypes = [vp, C.POINTER(BiasToken), C.c_int, C.POINTER(BiasKeyword), C.c_int, C.POINTER(C.c_int)]
    lib.dsm_asr_bias_create_text.argtypes = [vp, vp, C.POINTER(C.c_char_p), fp, C.c_int, C.POINTER(BiasToken), C.c_int, C.POINTER(C.c_int)]
    lib.dsm_asr_bias_destroy.argtypes = [vp, C.c_int]
    lib.dsm_asr_bias_info.argtypes = [vp, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_size_t)]
    lib.dsm_asr_set_bias.argtypes = [vp, C.c_int, C.c_int]
    lib.dsm_asr_bias_state.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    lib.dsm_text_bias_compile.argtypes = [C.POINTER(BiasToken), C.c_int, C.POINTER(BiasKeyword), C.c_int, C.c_int, u32p, C.c_size_t,
                                          C.POINTER(C.c_size_t)]
    lib.dsm_text_bias_pick_host.argtypes = [u32p, C.c_size_t, C.c_uint32, fp, C.c_int, C.c_float, u32p, C.c_uint64,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.dsm_debug_text_pick.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, u32p, C.c_float, u32p, vp, u32p, u32p]
    lib.dsm_worker_set_bias.argtypes = [vp, C.c_int, C.c_int]
    for name in ("dsm_asr_set_text_bias", "dsm_asr_bias_create", "dsm_asr_bias_create_text", "dsm_asr_bias_destroy", "dsm_asr_bias_info",
                 "dsm_asr_set_bias", "dsm_asr_bias_state", "dsm_text_bias_compile", "dsm_text_bias_pick_host", "dsm_debug_text_pick",
                 "dsm_worker_set_bias"):
        getattr(lib, name).restype = C.c_int
    for name in ("dsm_tts_create", "dsm_tts_step", "dsm_tts_audio_tokens", "dsm_tts_step_idx", "dsm_tts_reset_slot",
                 "dsm_tts_debug_read"):
        getattr(lib, name).restype = C.c_int
    intp = C.POINTER(C.c_int)
    lib.dsm_asr_set_ingest.argtypes = [vp, C.c_int]
    lib.dsm_asr_set_input_format.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.dsm_asr_input_format.argtypes = [vp, C.c_int] + [intp] * 5
    lib.dsm_mimi_encode_step_raw.argtypes = [vp, vp, C.c_size_t, vp, u32p, intp]
    lib.dsm_mimi_encode_step_raw_async.argtypes = [vp, vp, C.c_size_t, vp, intp]
    lib.dsm_mimi_encode_step_raw_dev.argtypes = [vp, vp, C.c_size_t, vp, vp]
    lib.dsm_asr_step_raw.argtypes = [vp, vp, C.c_size_t, vp, u32p, u32p, fp]
    lib.dsm_debug_ingest_read.argtypes = [vp, C.c_int, fp]
    lib.dsm_ingest_host_new.argtypes = [C.c_int, C.c_int]
    lib.dsm_ingest_host_new.restype = C.c_void_p
    lib.dsm_ingest_host_free.argtypes = [vp]
    lib.dsm_ingest_host_free.restype = None
    lib.dsm_ingest_host.argtypes = [vp, vp, fp]
    lib.dsm_ingest_describe.argtypes = [C.c_int, C.c_int, u32p]
    lib.dsm_ingest_g711_table.argtypes = [C.c_int, C.POINTER(C.c_int16)]
    lib.dsm_worker_set_input_rate.argtypes = [vp, C.c_int, C.c_int]
    for name in ("dsm_asr_set_ingest", "dsm_asr_set_input_format", "dsm_asr_input_format", "dsm_mimi_encode_step_raw",
                 "dsm_mimi_encode_step_raw_async", "dsm_mimi_encode_step_raw_dev", "dsm_asr_step_raw", "dsm_debug_ingest_read",
                 "dsm_ingest_host", "dsm_ingest_describe", "dsm_ingest_g711_table", "dsm_worker_set_input_rate"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_asr_set_clips.argtypes = [vp, C.c_int, C.c_size_t]
    lib.dsm_asr_clip_begin.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.dsm_asr_clip_push.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.dsm_asr_clip_close.argtypes = [vp, C.c_int]
    lib.dsm_asr_run.argtypes = [vp, C.c_int]
    lib.dsm_asr_collect.argtypes = [vp, C.POINTER(AsrBlockC)]
    lib.dsm_asr_clip_status.argtypes = [vp, C.c_int]
    lib.dsm_asr_clip_frame_host.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_uint64, vp]
    lib.dsm_asr_clip_host_new.argtypes = [C.c_int, C.c_size_t]
    lib.dsm_asr_clip_host_new.restype = C.c_void_p
    lib.dsm_asr_clip_host_free.argtypes = [vp]
    lib.dsm_asr_clip_host_free.restype = None
    lib.dsm_asr_clip_host_begin.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.dsm_asr_clip_host_push.argtypes = [vp, C.c_int, C.c_size_t]
    for name in ("dsm_asr_clip_host_close", "dsm_asr_clip_host_reset", "dsm_asr_clip_host_status"):
        getattr(lib, name).argtypes = [vp, C.c_int]
    lib.dsm_asr_clip_host_run.argtypes = [vp, C.c_int, vp, vp]
    for name in ("dsm_asr_set_clips", "dsm_asr_clip_begin", "dsm_asr_clip_push", "dsm_asr_clip_close", "dsm_asr_run", "dsm_asr_collect",
                 "dsm_asr_clip_status", "dsm_asr_clip_frame_host", "dsm_asr_clip_host_begin", "dsm_asr_clip_host_push",
                 "dsm_asr_clip_host_close", "dsm_asr_clip_host_reset", "dsm_asr_clip_host_status", "dsm_asr_clip_host_run"):
        getattr(lib, name).restype = C.c_int
    lib.dsm_tts_set_egress.argtypes = [vp, C.c_int]
    lib.dsm_tts_set_output_format.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.dsm_tts_output_format.argtypes = [vp, C.c_int] + [intp] * 5
    lib.dsm_tts_step_raw.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.dsm_tts_recv_raw.argtypes = [vp, vp, C.c_size_t, vp]
    lib.dsm_tts_collect_raw.argtypes = [vp, vp, vp, C.c_size_t]
    lib.dsm_tts_debug_egress.argtypes = [vp, vp, vp, vp, C.c_size_t]
    lib.dsm_egress_host_new.argtypes = [C.c_int, C.c_int]
    lib.dsm_egress_host_new.restype = C.c_void_p
    lib.dsm_egress_host_free.argtypes = [vp]
    lib.dsm_egress_host_free.restype = None
    lib.dsm_egress_host.argtypes = [vp, vp, vp]
    lib.dsm_egress_describe.argtypes = [C.c_int, C.c_int, u32p]
    lib.dsm_egress_encode_sample.argtypes = [C.c_int, C.c_float, vp]
    for name in ("dsm_tts_set_egress", "dsm_tts_set_output_format", "dsm_tts_output_format", "dsm_tts_step_raw", "dsm_tts_recv_raw",
                 "dsm_tts_collect_raw", "dsm_tts_debug_egress", "dsm_egress_host", "dsm_egress_describe", "dsm_egress_encode_sample"):
        getattr(lib, name).restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def config_stt_1b_en_fr():
    cfg = AsrConfig()
    load_library().dsm_asr_config_stt_1b_en_fr(C.byref(cfg))
    return cfg


def config_stt_2_6b_en():
    cfg = AsrConfig()
    load_library().dsm_asr_config_stt_2_6b_en(C.byref(cfg))
    return cfg


def config_tiny(kv_bf16=1):
    """A small configuration with every structural feature of stt-1b-en_fr (same ratios, T shapes,
    ring-cache wrap within a few steps) that the CPU oracle steps in milliseconds."""
    cfg = AsrConfig()
    t = cfg.lm
    t.d_model, t.num_heads, t.num_layers, t.dim_feedforward = 128, 4, 2, 512
    t.context, t.max_period, t.gating, t.norm = 12, 100000, 1, 1
    t.positional_embedding, t.layer_scale, t.conv_layout = 1, 0, 0
    cfg.text_in_vocab_size, cfg.text_out_vocab_size = 65, 64
    cfg.audio_vocab_size, cfg.audio_codebooks = 33, 4
    cfg.extra_heads_num, cfg.extra_heads_dim = 2, 6
    cfg.asr_delay_in_tokens, cfg.temperature, cfg.kv_bf16 = 2, 0.0, kv_bf16
    m = cfg.mimi
    m.channels, m.dimension, m.n_filters, m.n_residual_layers = 1, 64, 4, 1
    m.n_ratios = 4
    for i, r in enumerate((8, 6, 5, 4)):
        m.ratios[i] = r
    m.kernel_size, m.residual_kernel_size, m.last_kernel_size = 7, 3, 3
    m.dilation_base, m.compress = 2, 2
    mt = m.transformer
    mt.d_model, mt.num_heads, mt.num_layers, mt.dim_feedforward = 64, 2, 2, 128
    mt.context, mt.max_period, mt.gating, mt.norm = 10, 10000, 0, 0
    mt.positional_embedding, mt.layer_scale, mt.conv_layout = 1, 1, 1
    m.quantizer_n_q, m.quantizer_bins, m.quantizer_dim, m.downsample_stride = 4, 32, 16, 2
    return cfg


def config_medium(lm_heads=4, lm_head_dim=128, lm_context=300, kv_bf16=1, lm_layers=2, mimi_head_dim=64, mimi_context=250):
    """Between tiny and real: the LM and Mimi transformers get the REAL head dims (128 / 64) and ring lengths of a few
    hundred frames, so that the attention kernel's software-pipelined loop runs several iterations per phase (both
    register sets, the tail clamp after the first iteration, ring wrap) and d_model spans more than one 256-wide
    K-chunk (split-K slabs, the fused QKV prologue) — while SEANet, the RVQ and the vocabularies stay small enough for
    the CPU oracle to step a batch in ~10 ms."""
    cfg = config_tiny(kv_bf16)
    t = cfg.lm
    t.d_model, t.num_heads, t.num_layers = lm_heads * lm_head_dim, lm_heads, lm_layers
    t.dim_feedforward, t.context = 4 * t.d_model, lm_context  # gating hidden = 11 d / 4 (a multiple of 32 for d % 128 == 0)
    cfg.text_in_vocab_size, cfg.text_out_vocab_size = 257, 256
    cfg.audio_vocab_size, cfg.audio_codebooks = 65, 8
    cfg.asr_delay_in_tokens = 3
    m = cfg.mimi
    m.dimension, m.n_filters = 2 * mimi_head_dim, 4
    mt = m.transformer
    mt.d_model, mt.num_heads, mt.num_layers, mt.dim_feedforward, mt.context = 2 * mimi_head_dim, 2, 2, 256, mimi_context
    m.quantizer_n_q, m.quantizer_bins, m.quantizer_dim = 8, 64, 32
    return cfg


def config_tts_v202501():
    cfg = TtsConfig()
    load_library().dsm_tts_config_v202501(C.byref(cfg))
    return cfg


def config_tts_tiny(kv_bf16=1, cross_attention=False, cfg_rows=False, ca_dim=0, ca_norm=0):
    """Small TTS configuration with every structural feature of the v202501 model: shared depformer with
    fewer weight groups than slices, low-rank embeddings, acoustic and text-audio delays.  cross_attention / cfg_rows:
    the branch the reference server runs (norm_cross + cross-attention in every main-LM layer, two batch rows per slot)."""
    cfg = TtsConfig()
    t = cfg.lm
    t.d_model, t.num_heads, t.num_layers, t.dim_feedforward = 128, 4, 2, 512
    t.context, t.max_period, t.gating, t.norm = 16, 10000, 1, 1
    t.positional_embedding, t.layer_scale, t.conv_layout = 1, 0, 0
    cfg.text_in_vocab_size, cfg.text_out_vocab_size = 41, 40
    cfg.audio_vocab_size, cfg.audio_codebooks = 33, 6
    dp = cfg.depformer
    dp.d_model, dp.num_heads, dp.num_layers, dp.dim_feedforward = 64, 2, 2, 192
    dp.context, dp.max_period, dp.gating, dp.norm = 6, 10000, 1, 1
    dp.positional_embedding, dp.layer_scale, dp.conv_layout = 0, 0, 0
    cfg.dep_num_slices, cfg.dep_low_rank, cfg.dep_weight_groups = 6, 32, 3
    cfg.acoustic_delay, cfg.text_pad_token, cfg.text_bos_token = 2, 3, 1
    cfg.text_eos_token, cfg.text_eop_token, cfg.text_start_token = 2, 0, 40
    cfg.text_audio_delay_in_tokens, cfg.max_consecutive_pads, cfg.max_steps = 3, 4, 64
    cfg.kv_bf16 = kv_bf16
    if cross_attention:
        cfg.cross_attention, cfg.ca_norm, cfg.ca_dim, cfg.ca_max_len = 1, ca_norm, ca_dim, 24
        cfg.cfg_rows = 1 if cfg_rows else 0
    return cfg


def _blob_info(blob, info, call, last_error):
    """One of the two *_slot_blob_info calls on `blob`: the filled info struct as a dict, DsmError for a malformed blob."""
    lib = load_library()
    blob = bytes(blob)
    rc = getattr(lib, call)(blob, len(blob), C.byref(info))
    if rc < 0:
        msg = getattr(lib, last_error)(None)
        raise DsmError(f"dsm error {rc}: {msg.decode() if msg else '?'}")
    return {name: getattr(info, name) for name, _ in info._fields_ if name != "reserved"}


def slot_blob_info(blob):
    """dsm_slot_blob_info: header fields of a slot blob as a dict (host only, no device); DsmError for a malformed one."""
    return _blob_info(blob, SlotBlobInfo(), "dsm_slot_blob_info", "dsm_last_error")


def tts_slot_blob_info(blob):
    """dsm_tts_slot_blob_info: header fields of a TTS slot blob as a dict (host only, no device); DsmError for a malformed one."""
    return _blob_info(blob, TtsSlotBlobInfo(), "dsm_tts_slot_blob_info", "dsm_tts_last_error")


def tts_slot_layout(cfg, mimi_cfg=None):
    """dsm_tts_slot_layout: the device payload of a TTS slot blob for a configuration (host only, no device) as
    {"sections": [(name, bytes_per_slot, payload_offset), ...], "slot_bytes": int, "signature": [int, ...]};
    mimi_cfg None: without the Mimi decode group."""
    lib = load_library()
    mp = C.byref(mimi_cfg) if mimi_cfg is not None else None
    n = lib.dsm_tts_slot_layout(C.byref(cfg), mp, None, 0)
    if n < 0:
        msg = lib.dsm_tts_last_error(None)
        raise DsmError(f"dsm error {n}: {msg.decode() if msg else '?'}")
    buf = C.create_string_buffer(n + 1)
    lib.dsm_tts_slot_layout(C.byref(cfg), mp, buf, n + 1)
    out = {"sections": [], "slot_bytes": None, "signature": None}
    for line in buf.value.decode().splitlines():
        f = line.split()
        if f[0] == "slot_bytes":
            out["slot_bytes"] = int(f[1])
        elif f[0] == "signature":
            out["signature"] = [int(w) for w in f[1:]]
        else:
            out["sections"].append((f[0], int(f[1]), int(f[2])))
    return out


def token_scores_host(logits, token, top_n=0):
    """dsm_token_scores_host: (logprob of `token`, top ids [top_n] uint32, top logprobs [top_n] float32) of one row of f32
    logits, by the definition of csrc/dsm_token_scores.h computed serially on the host.  No device needed."""
    lib = load_library()
    row = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    lp = np.zeros(1, dtype=np.float32)
    n = max(int(top_n), 0)
    ids, lps = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32)
    token = int(token)
    if not 0 <= token < 2 ** 32:
        raise DsmError("token_scores_host: token outside uint32")
    rc = lib.dsm_token_scores_host(_ptr(row), row.size, token, int(top_n), _ptr(lp), _ptr(ids) if n else None, _ptr(lps) if n else None)
    if rc < 0:
        e = DsmError(f"dsm_token_scores_host: error {rc}")
        e.code = rc
        raise e
    return lp[0], ids, lps


def _bias_args(tokens, keywords):
    """((token, bias), ...), ((piece ids, boost), ...) -> the two C arrays with their counts, and what must stay alive."""
    tokens, keywords = list(tokens or ()), list(keywords or ())
    for t, _ in tokens:
        if not 0 <= int(t) < 2 ** 32:
            raise DsmError("text bias: token outside uint32")
    tk = (BiasToken * max(len(tokens), 1))(*[BiasToken(int(t), float(v)) for t, v in tokens])
    keep, kws = [], (BiasKeyword * max(len(keywords), 1))()
    for i, (ids, boost) in enumerate(keywords):
        a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        keep.append(a)
        kws[i] = BiasKeyword(a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None, a.size, float(boost))
    return tk, len(tokens), kws, len(keywords), keep


def _bias_fail(call, rc):
    e = DsmError(f"{call}: error {rc}: {load_library().dsm_last_error(None).decode(errors='replace')}")
    e.code = rc
    return e


def text_bias_compile(tokens, keywords, V):
    """dsm_text_bias_compile: the flat table (uint32 array, csrc/dsm_text_bias.h) of a bias set.  tokens: (token, bias) pairs,
    bias finite or -inf; keywords: (piece ids, boost) pairs, each ONE word.  Host only, no device needed."""
    lib = load_library()
    tk, nt, kws, nk, _keep = _bias_args(tokens, keywords)
    need = C.c_size_t(0)
    rc = lib.dsm_text_bias_compile(tk, nt, kws, nk, int(V), None, 0, C.byref(need))
    if rc < 0:
        raise _bias_fail("dsm_text_bias_compile", rc)
    out = np.zeros(need.value, dtype=np.uint32)
    rc = lib.dsm_text_bias_compile(tk, nt, kws, nk, int(V), _ptr(out), out.size, None)
    if rc < 0:
        raise _bias_fail("dsm_text_bias_compile", rc)
    return out


def text_bias_pick_host(table, node, logits, temperature=0.0, rng_key=None, rng_pos=0):
    """dsm_text_bias_pick_host: (token, next node) of one row of f32 logits by the definition of csrc/dsm_text_bias.h, computed
    serially on the host.  table: a compiled table, or None for "no set" (the node comes back unchanged)."""
    lib = load_library()
    row = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    t = None if table is None else np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
    key = None if rng_key is None else np.ascontiguousarray(rng_key, dtype=np.uint32).reshape(8)
    tok, nxt = C.c_uint32(0), C.c_uint32(0)
    rc = lib.dsm_text_bias_pick_host(_ptr(t), 0 if t is None else t.size, int(node), _ptr(row), row.size, float(temperature),
                                     _ptr(key), int(rng_pos), C.byref(tok), C.byref(nxt))
    if rc < 0:
        raise _bias_fail("dsm_text_bias_pick_host", rc)
    return tok.value, nxt.value


def _ptr(a):
    """Host pointer of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class DsmError(RuntimeError):
    pass


def encode_in_msg(kind, id=0, pcm=None, data=None):
    """InMsg -> msgpack bytes (client/rust/kyutai-client/src/stt/protocol.rs:47-58)."""
    lib = load_library()
    m = InMsg()
    m.kind, m.id = IN_KINDS.index(kind), id
    keep = []
    if pcm is not None:
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        keep.append(a)
        m.pcm, m.n_pcm = a.ctypes.data, a.size
    if data is not None:
        b = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        keep.append(b)
        m.data, m.n_data = b.ctypes.data, b.size
    n = lib.dsm_inmsg_encode(C.byref(m), None, 0)
    buf = np.zeros(max(n, 1), dtype=np.uint8)
    assert lib.dsm_inmsg_encode(C.byref(m), _ptr(buf), buf.size) == n
    return buf[:n].tobytes()


def decode_in_msg(raw):
    """msgpack bytes -> dict, as the server's rmp_serde::from_slice::<InMsg> (srv/batched_asr.rs:927); None if rejected."""
    lib = load_library()
    m = InMsg()
    pcm, data = np.zeros(len(raw) + 1, dtype=np.float32), np.zeros(len(raw) + 1, dtype=np.uint8)
    if lib.dsm_inmsg_decode(raw, len(raw), C.byref(m), _ptr(pcm), pcm.size, _ptr(data), data.size) != 0:
        return None
    out = {"type": IN_KINDS[m.kind]}
    if out["type"] == "Marker":
        out["id"] = m.id
    elif out["type"] == "Audio":
        out["pcm"] = pcm[:m.n_pcm].copy()
    elif out["type"] == "OggOpus":
        out["data"] = data[:m.n_data].tobytes()
    return out


def encode_out_msg(kind, text="", time=0.0, id=0, step_idx=0, prs=(), buffered_pcm=0):
    """OutMsg -> msgpack bytes, as send_loop serialises it (srv/batched_asr.rs:969-975)."""
    lib = load_library()
    m = OutMsg()
    p = np.ascontiguousarray(prs, dtype=np.float32)
    m.kind, m.text, m.time, m.id, m.step_idx = OUT_KINDS.index(kind), text.encode(), time, id, step_idx
    m.prs, m.n_prs, m.buffered_pcm = p.ctypes.data, p.size, buffered_pcm
    n = lib.dsm_outmsg_encode(C.byref(m), None, 0)
    buf = np.zeros(max(n, 1), dtype=np.uint8)
    assert lib.dsm_outmsg_encode(C.byref(m), _ptr(buf), buf.size) == n
    return buf[:n].tobytes()


def decode_out_msg(raw):
    """msgpack bytes -> dict (client: protocol.rs:60-62 decode_out_msg); None if rejected."""
    lib = load_library()
    m = OutMsg()
    text, prs = C.create_string_buffer(len(raw) + 1), np.zeros(len(raw) + 1, dtype=np.float32)
    if lib.dsm_outmsg_decode(raw, len(raw), C.byref(m), text, len(raw) + 1, _ptr(prs), prs.size) != 0:
        return None
    k = OUT_KINDS[m.kind]
    out = {"type": k}
    if k == "Word":
        out.update(text=text.value.decode(), start_time=m.time)
    elif k == "EndWord":
        out.update(stop_time=m.time)
    elif k == "Marker":
        out.update(id=m.id)
    elif k == "Step":
        out.update(step_idx=m.step_idx, prs=prs[:m.n_prs].tolist(), buffered_pcm=m.buffered_pcm)
    elif k == "Error":
        out.update(message=text.value.decode())
    return out


class Tokenizer:
    """The native SentencePiece tokenizer (dsm_spm_*, csrc/dsm_spm.h): a UNIGRAM model from a path or from the file's bytes.
    encode / decode answer byte for byte what sentencepiece.SentencePieceProcessor does with the same file; text crosses as
    UTF-8 bytes (a str is encoded first), decode returns bytes."""

    def __init__(self, model):
        self.lib = load_library()
        h = C.c_void_p()
        if isinstance(model, (bytes, bytearray, memoryview)):
            raw = bytes(model)
            rc = self.lib.dsm_spm_load_bytes(raw, len(raw), C.byref(h))
        else:
            rc = self.lib.dsm_spm_load(os.fsencode(model), C.byref(h))
        if rc != 0:
            e = DsmError(f"dsm error {rc}: {self.lib.dsm_spm_last_error(None).decode(errors='replace')}")
            e.code = rc
            raise e
        self.h = h

    @property
    def vocab_size(self):
        return self.lib.dsm_spm_vocab_size(self.h)

    @property
    def special_ids(self):
        """(unk, bos, eos, pad); -1 where the model has none."""
        v = [C.c_int(-1) for _ in range(4)]
        self.lib.dsm_spm_special_ids(self.h, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def encode(self, text):
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        ids = np.zeros(max(8, 2 * len(raw) + 8), dtype=np.uint32)
        n = self.lib.dsm_spm_encode(self.h, raw, len(raw), _ptr(ids), ids.size)
        if n > ids.size:  # the call wrote nothing: it tells the size
            ids = np.zeros(n, dtype=np.uint32)
            n = self.lib.dsm_spm_encode(self.h, raw, len(raw), _ptr(ids), ids.size)
        return [int(x) for x in ids[:n]]

    def decode(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        n = self.lib.dsm_spm_decode(self.h, _ptr(a) if a.size else None, a.size, None, 0)
        if n < 0:
            e = DsmError(f"dsm error {n}: {self.lib.dsm_spm_last_error(self.h).decode(errors='replace')}")
            e.code = int(n)
            raise e
        out = C.create_string_buffer(max(1, n))
        self.lib.dsm_spm_decode(self.h, _ptr(a) if a.size else None, a.size, out, n)
        return out.raw[:n]

    def close(self):
        if getattr(self, "h", None):
            self.lib.dsm_spm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Worker:
    """moshi-server's BatchedAsr module above an AsrEngine, minus the sockets: slot table, per-channel PCM queue,
    markers, message fan-out (srv/batched_asr.rs).  Messages cross this interface as the msgpack bytes of the wire."""

    def __init__(self, engine=None, detokenizer=None, backend=None, tokenizer_file=None):
        """engine: an AsrEngine (the product path).  backend: a filled WorkerBackend instead (the tests drive the
        worker logic with the CPU oracle through it); the caller keeps its callbacks alive.  tokenizer_file: a SentencePiece
        model for Word.text (dsm_worker_set_tokenizer_file); a detokenizer callback, if given too, wins."""
        self.lib, self.engine, self.backend = load_library(), engine, backend
        h = C.c_void_p()
        if backend is not None:
            rc = self.lib.dsm_worker_create_with_backend(C.byref(backend), C.byref(h))
        else:
            rc = self.lib.dsm_worker_create(engine.h, C.byref(h))
        if rc != 0:
            raise DsmError("dsm_worker_create failed")
        self.h = h
        self._cb = None
        if detokenizer is not None:
            def cb(_user, toks, n, out, cap):
                s = detokenizer([toks[i] for i in range(n)]).encode()
                if len(s) > cap:
                    return -1
                C.memmove(out, s, len(s))
                return len(s)
            self._cb = DETOK_FN(cb)
            self.lib.dsm_worker_set_detokenizer(self.h, self._cb, None)
        if tokenizer_file is not None:
            self.set_tokenizer_file(tokenizer_file)

    def set_tokenizer_file(self, path):
        rc = self.lib.dsm_worker_set_tokenizer_file(self.h, os.fsencode(path))
        if rc < 0:
            e = DsmError(f"dsm error {rc}: {self._err()}")
            e.code = rc
            raise e

    def set_word_scores(self, on):
        """dsm_worker_set_word_scores: Word messages carry logprob / min_logprob (mean and minimum of the word's token
        log-probabilities).  Engine-backed workers only."""
        rc = self.lib.dsm_worker_set_word_scores(self.h, 1 if on else 0)
        if rc < 0:
            e = DsmError(f"dsm error {rc}: {self._err()}")
            e.code = rc
            raise e

    def set_input_rate(self, slot, hz):
        """dsm_worker_set_input_rate: the open channel's Audio samples are f32 at `hz` from now on (set before its first audio);
        its queue is cut into frames of 2 hz / 25 samples and resampled on the device.  24000 again when the channel closes.
        Engine-backed workers only."""
        rc = self.lib.dsm_worker_set_input_rate(self.h, int(slot), int(hz))
        if rc < 0:
            e = DsmError(f"dsm error {rc}: {self._err()}")
            e.code = rc
            raise e

    def set_bias(self, slot, handle):
        """dsm_worker_set_bias: attach an open channel's slot to a bias set of the engine (0 detaches); the worker detaches it
        when the channel closes.  Engine-backed workers only."""
        rc = self.lib.dsm_worker_set_bias(self.h, int(slot), int(handle or 0))
        if rc < 0:
            e = DsmError(f"dsm error {rc}: {self._err()}")
            e.code = rc
            raise e

    def _err(self):
        return self.lib.dsm_worker_last_error(self.h).decode()

    def open(self):
        cid = C.c_uint64(0)
        slot = self.lib.dsm_worker_open(self.h, C.byref(cid))
        if slot < 0:
            raise DsmError(self._err())
        return slot

    def close_channel(self, slot):
        self.lib.dsm_worker_close(self.h, slot)

    def send(self, slot, raw):
        rc = self.lib.dsm_worker_send(self.h, slot, raw, len(raw))
        if rc < 0:
            raise DsmError(self._err())
        return rc == 0

    def send_body(self, slot, body):
        """BatchedAsr::handle_query: a whole audio file as the request (Init, the clip at 24 kHz, Marker 0, 10 s of silence)."""
        rc = self.lib.dsm_worker_send_body(self.h, slot, body, len(body))
        if rc < 0:
            raise DsmError(self._err())

    def step(self):
        rc = self.lib.dsm_worker_step(self.h)
        if rc < 0:
            raise DsmError(self._err())
        return rc == 1

    def step_encode(self):
        """encoder_loop iteration (dsm_worker_step_encode): True if a frame was cut and queued for the model side."""
        rc = self.lib.dsm_worker_step_encode(self.h)
        if rc < 0:
            raise DsmError(self._err())
        return rc == 1

    def step_model(self):
        """model_loop + post_process for the oldest queued frame (dsm_worker_step_model)."""
        rc = self.lib.dsm_worker_step_model(self.h)
        if rc < 0:
            raise DsmError(self._err())
        return rc == 1

    def recv(self, slot):
        """All pending OutMsg of the slot, decoded."""
        out, buf, n = [], np.zeros(1 << 16, dtype=np.uint8), C.c_size_t(0)
        while self.lib.dsm_worker_recv(self.h, slot, _ptr(buf), buf.size, C.byref(n)) == 1:
            out.append(decode_out_msg(buf[:n.value].tobytes()))
        return out

    def buffered(self, slot):
        return self.lib.dsm_worker_buffered(self.h, slot)

    def close(self):
        if getattr(self, "h", None):
            self.lib.dsm_worker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mp3Info(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("channels", C.c_int), ("bitrate_kbps", C.c_int), ("vbr", C.c_int), ("frames", C.c_int),
                ("info_frames", C.c_int), ("resyncs", C.c_int), ("huffman_overruns", C.c_int), ("frames_without_reservoir", C.c_int),
                ("id3v2_bytes", C.c_uint64), ("junk_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _take_pcm(lib, ptr, n):
    try:
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        lib.dsm_free(ptr)


def mp3_decode(data):
    """(pcm f32 of channel 0, sample_rate, info dict) of an MPEG-1 Layer III body — srv/utils.rs:263-305 pcm_decode (symphonia)."""
    lib = load_library()
    ptr, n, info = C.POINTER(C.c_float)(), C.c_size_t(0), Mp3Info()
    rc = lib.dsm_mp3_decode_info(data, len(data), C.byref(ptr), C.byref(n), C.byref(info))
    if rc != 0:
        msg = lib.dsm_last_error(None)
        raise DsmError(f"dsm_mp3_decode failed ({rc}): {msg.decode() if msg else '?'}")
    return _take_pcm(lib, ptr, n), info.sample_rate, info.as_dict()


def mp3_probe(data):
    lib = load_library()
    info = Mp3Info()
    rc = lib.dsm_mp3_probe(data, len(data), C.byref(info))
    if rc != 0:
        msg = lib.dsm_last_error(None)
        raise DsmError(f"dsm_mp3_probe failed ({rc}): {msg.decode() if msg else '?'}")
    return info.as_dict()


def pcm_decode(data):
    """RIFF/WAVE or mp3 by magic: (pcm of channel 0, sample_rate) — what the worker front end does with a request body."""
    lib = load_library()
    ptr, n, rate = C.POINTER(C.c_float)(), C.c_size_t(0), C.c_int(0)
    rc = lib.dsm_pcm_decode(data, len(data), C.byref(ptr), C.byref(n), C.byref(rate))
    if rc != 0:
        msg = lib.dsm_last_error(None)
        raise DsmError(f"dsm_pcm_decode failed ({rc}): {msg.decode() if msg else '?'}")
    return _take_pcm(lib, ptr, n), rate.value


def resample(pcm, rate_in, rate_out):
    """Whole-buffer windowed-sinc resampler in the place of kaudio::resample (srv/batched_asr.rs:838)."""
    lib = load_library()
    x = np.ascontiguousarray(pcm, dtype=np.float32)
    ptr, n = C.POINTER(C.c_float)(), C.c_size_t(0)
    rc = lib.dsm_resample(x.ctypes.data, x.size, int(rate_in), int(rate_out), C.byref(ptr), C.byref(n))
    if rc != 0:
        raise DsmError(f"dsm_resample failed ({rc})")
    return _take_pcm(lib, ptr, n)


def wav_decode(data):
    """(pcm f32 of channel 0, sample_rate) of a RIFF/WAVE body — srv/utils.rs:263-305 pcm_decode."""
    lib = load_library()
    ptr, n, rate = C.POINTER(C.c_float)(), C.c_size_t(0), C.c_int(0)
    rc = lib.dsm_wav_decode(data, len(data), C.byref(ptr), C.byref(n), C.byref(rate))
    if rc != 0:
        msg = lib.dsm_last_error(None)
        raise DsmError(f"dsm_wav_decode failed ({rc}): {msg.decode() if msg else '?'}")
    try:
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32), rate.value
    finally:
        lib.dsm_free(ptr)


def _pcm_describe(call, frame_key, rate, fmt):
    """dsm_ingest_describe / dsm_egress_describe: the twelve descriptor words of a format (csrc/dsm_pcm_format.h) as a dict, the
    frame length under the direction's own key, without the table offset and the reserved word."""
    lib = load_library()
    w = np.zeros(12, dtype=np.uint32)
    rc = getattr(lib, call)(int(rate), int(fmt), _ptr(w))
    if rc != 0:
        msg = lib.dsm_last_error(None)
        raise DsmError(f"{call} failed ({rc}): {msg.decode() if msg else '?'}")
    names = ("rate", "fmt", "L", "M", "half", "taps", frame_key, "frame_bytes", "D", "table_off", "table_words", "reserved")
    return {k: int(v) for k, v in zip(names, w) if k not in ("table_off", "reserved")}


def ingest_describe(rate, fmt):
    """dsm_ingest_describe: the descriptor of an input format (csrc/dsm_pcm_format.h, DSM_PCM_IN) as a dict — rate, fmt, L, M,
    half, taps, F_in, frame_bytes, D (the latency in 24 kHz samples), table_words.  DsmError with the reason for a rate or format
    outside the definition."""
    return _pcm_describe("dsm_ingest_describe", "F_in", rate, fmt)


def ingest_g711_table(fmt):
    """The 256 expanded 16-bit values of PCM_MULAW / PCM_ALAW (int16 array), as the engine's tables are built."""
    out = np.zeros(256, dtype=np.int16)
    if load_library().dsm_ingest_g711_table(int(fmt), out.ctypes.data_as(C.POINTER(C.c_int16))) != 0:
        raise DsmError("dsm_ingest_g711_table: the format is neither mu-law nor A-law")
    return out


class _pcm_host:
    """What ingest_host and egress_host share: the format's descriptor, the C state and its release.  A subclass names its
    calls (`_side`) and its describe function's frame key, and adds step()."""
    _side = _frame_key = None

    def __init__(self, rate, fmt=PCM_F32):
        self.lib = load_library()
        self.info = _pcm_describe(f"dsm_{self._side}_describe", self._frame_key, rate, fmt)  # raises with the reason for an unsupported format
        self.frame_samples, self.frame_bytes, self.latency = self.info[self._frame_key], self.info["frame_bytes"], self.info["D"]
        self.h = getattr(self.lib, f"dsm_{self._side}_host_new")(int(rate), int(fmt))
        if not self.h:
            msg = self.lib.dsm_last_error(None)
            raise DsmError(f"dsm_{self._side}_host_new failed: {msg.decode() if msg else '?'}")

    def _step(self, src, out):
        rc = getattr(self.lib, f"dsm_{self._side}_host")(self.h, src, _ptr(out))
        if rc != 0:
            msg = self.lib.dsm_last_error(None)
            raise DsmError(f"dsm_{self._side}_host failed ({rc}): {msg.decode() if msg else '?'}")
        return out

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, f"dsm_{self._side}_host_free")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ingest_host(_pcm_host):
    """dsm_ingest_host_*: one slot's streaming ingest on the host — the function ingest_resample_kernel is bit-identical to.
    step(raw) takes one frame (bytes, or an array whose bytes are the frame: frame_bytes of them) and returns the 1920 samples
    at 24 kHz the step hands Mimi."""
    _side, _frame_key = "ingest", "F_in"

    def step(self, raw):
        raw = raw if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).tobytes()
        if len(raw) != self.frame_bytes:
            raise DsmError(f"ingest_host.step: a frame of {len(raw)} bytes, the format's frame has {self.frame_bytes}")
        return self._step(bytes(raw), np.zeros(FRAME_SIZE, dtype=np.float32))


def egress_describe(rate, fmt):
    """dsm_egress_describe: the descriptor of an output format (csrc/dsm_pcm_format.h, DSM_PCM_OUT) as a dict — rate, fmt, L, M,
    half, taps, F_out, frame_bytes, D (the latency in output samples), table_words.  DsmError with the reason for a rate or
    format outside the definition."""
    return _pcm_describe("dsm_egress_describe", "F_out", rate, fmt)


def egress_encode_sample(fmt, v):
    """dsm_egress_encode_sample: one sample through the shared encoder — the f32 bits (uint32), the s16 value, or the G.711 byte."""
    out = np.zeros(4, dtype=np.uint8)
    if load_library().dsm_egress_encode_sample(int(fmt), C.c_float(v), _ptr(out)) != 0:
        raise DsmError("dsm_egress_encode_sample: the format is none of DSM_PCM_*")
    if fmt == PCM_F32:
        return int(out.view("<u4")[0])
    return int(out[:2].view("<i2")[0]) if fmt == PCM_S16 else int(out[0])


class egress_host(_pcm_host):
    """dsm_egress_host_*: one slot's streaming egress on the host — the function egress_resample_kernel is bit-identical to.
    step(frame) takes one emitted frame of 1920 f32 samples at 24 kHz and returns the format's frame as frame_bytes uint8."""
    _side, _frame_key = "egress", "F_out"

    def step(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        if frame.size != FRAME_SIZE:
            raise DsmError(f"egress_host.step: a frame of {frame.size} samples, a step has {FRAME_SIZE}")
        return self._step(_ptr(frame), np.zeros(self.frame_bytes, dtype=np.uint8))


def asr_clip_frame_host(clip, rate, fmt, index):
    """dsm_asr_clip_frame_host: frame `index` of a clip (bytes in the format (rate, fmt)) as bytes — the clip's bytes
    [index * frame_bytes, (index + 1) * frame_bytes) followed by the format's silence byte (csrc/dsm_asr_clip.h)."""
    clip = bytes(clip)
    out = np.zeros(INGEST_MAX_FRAME_BYTES, dtype=np.uint8)
    src = np.frombuffer(clip, dtype=np.uint8) if clip else None
    n = load_library().dsm_asr_clip_frame_host(_ptr(src), len(clip), int(rate), int(fmt), int(index), _ptr(out))
    if n < 0:
        msg = load_library().dsm_last_error(None)
        raise DsmError(f"dsm_asr_clip_frame_host: {msg.decode() if msg else '?'}")
    return out[:n].tobytes()


class asr_clip_host:
    """dsm_asr_clip_host_*: the schedule dsm_asr_run goes through, on the host alone — B slots, a cap per clip; begin / push (a
    byte count) / close / reset / status as the engine's, run(n) -> (frame [n][B] u32, mask [n][B] u8)."""

    def __init__(self, B, max_clip_bytes):
        self.lib, self.B = load_library(), int(B)
        self.h = self.lib.dsm_asr_clip_host_new(self.B, int(max_clip_bytes))
        if not self.h:
            raise DsmError("dsm_asr_clip_host_new: a batch size below 1 or a cap outside 1 .. 2^31")

    def _check(self, rc, what):
        if rc < 0:
            raise DsmError(f"dsm_asr_clip_host_{what}: error {rc}")
        return rc

    def begin(self, slot, rate, fmt, flush_frames):
        self._check(self.lib.dsm_asr_clip_host_begin(self.h, int(slot), int(rate), int(fmt), int(flush_frames)), "begin")

    def push(self, slot, n):
        self._check(self.lib.dsm_asr_clip_host_push(self.h, int(slot), int(n)), "push")

    def close(self, slot):
        self._check(self.lib.dsm_asr_clip_host_close(self.h, int(slot)), "close")

    def reset(self, slot):
        self._check(self.lib.dsm_asr_clip_host_reset(self.h, int(slot)), "reset")

    def status(self, slot):
        return self._check(self.lib.dsm_asr_clip_host_status(self.h, int(slot)), "status")

    def run(self, n_steps):
        n = int(n_steps)
        frame, mask = np.zeros((max(n, 1), self.B), dtype=np.uint32), np.zeros((max(n, 1), self.B), dtype=np.uint8)
        self._check(self.lib.dsm_asr_clip_host_run(self.h, n, _ptr(frame), _ptr(mask)), "run")
        return frame, mask

    def free(self):
        if getattr(self, "h", None):
            self.lib.dsm_asr_clip_host_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class LinearResampler:
    """kyutai-client-core `LinearResampler` (audio.rs:133-183) behind the C ABI; process() is streaming."""

    def __init__(self, in_rate_hz, out_rate_hz):
        self.lib = load_library()
        self.h = self.lib.dsm_linear_resampler_new(in_rate_hz, out_rate_hz)
        if not self.h:
            raise DsmError("bad sample rates")
        self.ratio = out_rate_hz / in_rate_hz

    def process(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        out = np.zeros(int(pcm.size * self.ratio) + 4, dtype=np.float32)
        n = self.lib.dsm_linear_resampler_process(self.h, _ptr(pcm), pcm.size, _ptr(out), out.size)
        assert n <= out.size
        return out[:n]

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dsm_linear_resampler_free(self.h)
            self.h = None


class AsrEngine:
    """Mirror of the reference's (Mimi::batched, LmModel::batched, asr::State) triple behind the C ABI.

    Method names follow the reference: encode_step (core/mimi.rs:195), step_tokens (core/asr.rs:147),
    step_pcm (core/asr.rs:115), reset_batch_idx (core/asr.rs:257)."""

    def __init__(self, cfg, batch_size, lm_path=None, mimi_path=None, device_id=0, arena=None):
        """From the two safetensors files, or — `arena=(device_ptr, nbytes, manifest_bytes[, keepalive])` — attached to a
        packed weight arena another rank broadcast (dsm_asr_create_from_arena); the caller's buffer must outlive the engine
        (pass it as the optional 4th element and it is kept referenced here)."""
        self.lib = load_library()
        self.cfg = cfg
        self.B = batch_size
        h = C.c_void_p()
        if arena is not None:
            ptr, nbytes, manifest = arena[0], arena[1], bytes(arena[2])
            self._arena_keepalive = arena[3] if len(arena) > 3 else None
            mbuf = (C.c_uint8 * max(len(manifest), 1)).from_buffer_copy(manifest or b"\0")
            rc = self.lib.dsm_asr_create_from_arena(C.byref(cfg), device_id, batch_size, C.c_void_p(ptr), nbytes, mbuf,
                                                    len(manifest), C.byref(h))
        else:
            rc = self.lib.dsm_asr_create(C.byref(cfg), device_id, batch_size, lm_path.encode(), mimi_path.encode(),
                                         C.byref(h))
        if rc != 0:
            msg = self.lib.dsm_last_error(None)
            raise DsmError(f"dsm_asr_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.h = h
        self.n_q = self.lib.dsm_n_q(h)

    @classmethod
    def replica(cls, src, device_id, batch_size=None, cfg=None):
        """A second engine in THIS process on `device_id` whose weights are a device-to-device copy of `src`'s arena
        (dsm_asr_create_replica: hipMemcpyPeerAsync over xGMI; a device copy when device_id is src's own device)."""
        self = cls.__new__(cls)
        self.lib = src.lib
        self.cfg = cfg if cfg is not None else src.cfg
        self.B = batch_size if batch_size is not None else src.B
        h = C.c_void_p()
        rc = self.lib.dsm_asr_create_replica(src.h, C.byref(self.cfg) if cfg is not None else None, device_id, self.B, C.byref(h))
        if rc != 0:
            msg = self.lib.dsm_last_error(None)
            raise DsmError(f"dsm_asr_create_replica failed ({rc}): {msg.decode() if msg else '?'}")
        self.h = h
        self.n_q = self.lib.dsm_n_q(h)
        return self

    def weight_arena(self):
        """(device pointer, nbytes, manifest bytes) of this engine's packed weight arena (dsm_asr_weight_arena)."""
        ptr, n, mp, mn = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self.lib.dsm_asr_weight_arena(self.h, C.byref(ptr), C.byref(n), C.byref(mp), C.byref(mn)))
        manifest = C.string_at(mp, mn.value) if mn.value else b""
        return ptr.value, n.value, manifest

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.dsm_last_error(self.h)
            raise DsmError(f"dsm error {rc}: {msg.decode() if msg else '?'}")
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.dsm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_step(self, pcm, mask):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(self.B, FRAME_SIZE)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        codes = np.zeros((self.B, self.n_q), dtype=np.uint32)
        produced = C.c_int(0)
        self._check(self.lib.dsm_mimi_encode_step(self.h, _ptr(pcm), _ptr(mask), _ptr(codes), C.byref(produced)))
        return codes if produced.value else None

    def decode_step(self, codes, mask):
        codes = np.ascontiguousarray(codes, dtype=np.uint32).reshape(self.B, self.n_q)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        pcm = np.zeros((self.B, FRAME_SIZE), dtype=np.float32)
        produced = C.c_int(0)
        self._check(self.lib.dsm_mimi_decode_step(self.h, _ptr(codes), _ptr(mask), _ptr(pcm), C.byref(produced)))
        return pcm if produced.value else None

    def decode_step_dev(self, d_codes, d_mask, d_pcm):
        self._check(self.lib.dsm_mimi_decode_step_dev(self.h, d_codes, d_mask, d_pcm))

    def step_tokens(self, codes, mask):
        """codes None: use the device-resident codes of the last encode_step (srv/batched_asr.rs hands them over on-device too)."""
        if codes is not None:
            codes = np.ascontiguousarray(codes, dtype=np.uint32).reshape(self.B, self.n_q)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        text = np.zeros(self.B, dtype=np.uint32)
        nh = self.cfg.extra_heads_num
        prs = np.zeros((max(nh, 1), self.B), dtype=np.float32)
        self._check(self.lib.dsm_asr_step_tokens(self.h, _ptr(codes), _ptr(mask), _ptr(text), _ptr(prs) if nh else None))
        return text, prs[:nh]

    def step_pcm(self, pcm, mask):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(self.B, FRAME_SIZE)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        codes = np.zeros((self.B, self.n_q), dtype=np.uint32)
        text = np.zeros(self.B, dtype=np.uint32)
        nh = self.cfg.extra_heads_num
        prs = np.zeros((max(nh, 1), self.B), dtype=np.float32)
        self._check(self.lib.dsm_asr_step_pcm(self.h, _ptr(pcm), _ptr(mask), _ptr(codes), _ptr(text),
                                              _ptr(prs) if nh else None))
        return codes, text, prs[:nh]

    def poll_msgs(self, cap=4096):
        msgs = (AsrMsg * cap)()
        toks = np.zeros(cap * 8, dtype=np.uint32)
        n = self._check(self.lib.dsm_asr_poll_msgs(self.h, msgs, cap, _ptr(toks), toks.size))
        out = []
        for i in range(n):
            m = msgs[i]
            if m.kind == MSG_WORD:
                out.append(("Word", m.batch_idx, m.time, toks[m.tokens_offset:m.tokens_offset + m.n_tokens].tolist()))
            elif m.kind == MSG_END_WORD:
                out.append(("EndWord", m.batch_idx, m.time))
            else:
                out.append(("Step", m.step_idx))
        return out

    # token scores (include/dsm.h "token scores")
    def set_token_scores(self, top_n):
        """-1 (or None): off, the default.  0..8: every step also yields the log-probability of each slot's text token and
        the top_n best entries of its logits row."""
        self._check(self.lib.dsm_asr_set_token_scores(self.h, -1 if top_n is None else int(top_n)))

    def token_scores(self):
        """Scores of the last step_tokens / step_pcm / step_tokens_ticket: (logprob [B] f32, top_ids [B, top_n] u32,
        top_logprobs [B, top_n] f32)."""
        lp = np.zeros(self.B, dtype=np.float32)
        ids = np.zeros((self.B, SCORES_MAX_TOP), dtype=np.uint32)
        lps = np.zeros((self.B, SCORES_MAX_TOP), dtype=np.float32)
        n = self._check(self.lib.dsm_asr_token_scores(self.h, _ptr(lp), _ptr(ids), _ptr(lps)))
        # the library wrote [B][top_n] densely into the front of the two buffers
        return lp, ids.reshape(-1)[:self.B * n].reshape(self.B, n).copy(), lps.reshape(-1)[:self.B * n].reshape(self.B, n).copy()

    def token_scores_dev(self):
        """(top_n, device pointers of logprob [B], top_ids [B, 8], top_logprobs [B, 8]) for the *_dev callers: valid after
        sync(), overwritten by the next step."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = self._check(self.lib.dsm_asr_token_scores_dev(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return n, a.value, b.value, c.value

    def poll_word_scores(self, cap=4096 * 8):
        """Parallel to poll_msgs' tokens: float32 array whose entries [tokens_offset, tokens_offset + n_tokens) are a Word's
        token log-probabilities (NaN = not recorded).  Use word_scores() for them per message."""
        out = np.zeros(cap, dtype=np.float32)
        n = self._check(self.lib.dsm_asr_poll_word_scores(self.h, _ptr(out), cap))
        return out[:n]

    def word_scores(self, cap=4096):
        """[(batch_idx, [logprob of each token]), ...] for the Word messages of the last step, in poll_msgs order."""
        msgs = (AsrMsg * cap)()
        n = self._check(self.lib.dsm_asr_poll_msgs(self.h, msgs, cap, None, 0))
        lps = self.poll_word_scores(cap * 8)
        return [(msgs[i].batch_idx, lps[msgs[i].tokens_offset:msgs[i].tokens_offset + msgs[i].n_tokens].copy())
                for i in range(n) if msgs[i].kind == MSG_WORD]

    def debug_token_scores(self, logits, tokens, top_n):
        """Test aid: the step's score KERNEL on caller-supplied rows.  logits [n, V] f32, tokens [n] -> (logprob [n],
        top_ids [n, top_n], top_logprobs [n, top_n])."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        n, V = logits.shape
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32).reshape(n)
        k = int(top_n)
        lp = np.zeros(n, dtype=np.float32)
        ids, lps = np.zeros((n, max(k, 0)), dtype=np.uint32), np.zeros((n, max(k, 0)), dtype=np.float32)
        self._check(self.lib.dsm_debug_token_scores(self.h, _ptr(logits), n, V, _ptr(tokens), k, _ptr(lp),
                                                    _ptr(ids) if k > 0 else None, _ptr(lps) if k > 0 else None))
        return lp, ids, lps

    # text bias (include/dsm.h "text bias")
    def set_text_bias(self, on):
        """Engine-wide switch, off by default: on, every slot's text token is picked by lm_pick_biased_kernel over the raw
        logits plus the biases of the set the slot is attached to."""
        self._check(self.lib.dsm_asr_set_text_bias(self.h, 1 if on else 0))

    def bias_create(self, tokens=(), keywords=()):
        """tokens: (token, bias) pairs, bias finite or -inf (a ban); keywords: (piece ids, boost) pairs, each ONE word.
        Returns the set's handle (positive, never reused)."""
        tk, nt, kws, nk, _keep = _bias_args(tokens, keywords)
        h = C.c_int(0)
        self._check(self.lib.dsm_asr_bias_create(self.h, tk, nt, kws, nk, C.byref(h)))
        return h.value

    def bias_create_text(self, tokenizer, words, boosts, tokens=()):
        """The keywords as text: each word is encoded alone with `tokenizer` (a Tokenizer)."""
        words = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words]
        arr = (C.c_char_p * max(len(words), 1))(*words)
        b = np.ascontiguousarray(boosts, dtype=np.float32).reshape(-1)
        if b.size != len(words):
            raise DsmError("bias_create_text: one boost per word")
        tk, nt, _, _, _keep = _bias_args(tokens, ())
        h = C.c_int(0)
        self._check(self.lib.dsm_asr_bias_create_text(self.h, tokenizer.h, arr, _ptr(b), len(words), tk, nt, C.byref(h)))
        return h.value

    def bias_destroy(self, handle):
        self._check(self.lib.dsm_asr_bias_destroy(self.h, int(handle)))

    def bias_info(self, handle):
        """dict(nodes, edges, tokens, refs, device_bytes) of a set."""
        v = [C.c_int(0) for _ in range(4)]
        nbytes = C.c_size_t(0)
        self._check(self.lib.dsm_asr_bias_info(self.h, int(handle), *[C.byref(x) for x in v], C.byref(nbytes)))
        return dict(nodes=v[0].value, edges=v[1].value, tokens=v[2].value, refs=v[3].value, device_bytes=nbytes.value)

    def set_bias(self, slot, handle):
        """Attach `slot` to a set; 0 (or None) detaches."""
        self._check(self.lib.dsm_asr_set_bias(self.h, int(slot), int(handle or 0)))

    def bias_state(self, slot):
        """(set handle or 0, trie node) of the slot as of the last finished step."""
        s, n = C.c_int(0), C.c_uint32(0)
        self._check(self.lib.dsm_asr_bias_state(self.h, int(slot), C.byref(s), C.byref(n)))
        return s.value, n.value

    def debug_text_pick(self, handle, logits, nodes, temperature=0.0, rng_keys=None, rng_pos=None):
        """Test aid: the step's pick KERNEL on caller-supplied rows.  logits [n, V] f32, nodes [n]; for temperature > 0 rng_keys
        [n, 8] u32 and rng_pos [n] u64 -> (tokens [n] u32, next nodes [n] u32)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        n, V = logits.shape
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(n)
        keys = None if rng_keys is None else np.ascontiguousarray(rng_keys, dtype=np.uint32).reshape(n, 8)
        pos = None if rng_pos is None else np.ascontiguousarray(rng_pos, dtype=np.uint64).reshape(n)
        toks, nxt = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._check(self.lib.dsm_debug_text_pick(self.h, int(handle or 0), _ptr(logits), n, V, _ptr(nodes), float(temperature),
                                                 _ptr(keys), _ptr(pos), _ptr(toks), _ptr(nxt)))
        return toks, nxt

    def reset_batch_idx(self, slot):
        self._check(self.lib.dsm_asr_reset_slot(self.h, slot))

    def mimi_reset_batch_idx(self, slot):
        self._check(self.lib.dsm_mimi_reset_slot(self.h, slot))

    def sync(self):
        self._check(self.lib.dsm_sync(self.h))

    def metrics(self):
        m = Metrics()
        self._check(self.lib.dsm_get_metrics(self.h, C.byref(m)))
        return m

    def debug_read(self, name, n):
        out = np.zeros(n, dtype=np.float32)
        got = self._check(self.lib.dsm_debug_read(self.h, name.encode(), _ptr(out), n))
        return out[:got]

    # ingest (include/dsm.h "ingest"): per-slot input sample rate and sample format, resampled on the device
    def set_ingest(self, on):
        """dsm_asr_set_ingest: the engine-wide switch; on allocates the section and lets the raw calls run."""
        self._check(self.lib.dsm_asr_set_ingest(self.h, 1 if on else 0))

    def set_input_format(self, slot, rate, fmt=PCM_F32):
        """dsm_asr_set_input_format: the slot's format from its next frame on; clears its history on both Mimi sides."""
        self._check(self.lib.dsm_asr_set_input_format(self.h, int(slot), int(rate), int(fmt)))

    def input_format(self, slot):
        """(rate, fmt, frame_samples, frame_bytes, latency in 24 kHz samples) of the slot."""
        v = [C.c_int(0) for _ in range(5)]
        self._check(self.lib.dsm_asr_input_format(self.h, int(slot), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _raw_rows(self, raw, pitch):
        """raw: bytes / a uint8 array of B * pitch bytes, or a list of B per-slot frames (bytes or arrays) packed here."""
        if isinstance(raw, (list, tuple)):
            rows = np.zeros((self.B, pitch), dtype=np.uint8)
            for b, r in enumerate(raw):
                if r is None:
                    continue
                r = np.frombuffer(r if isinstance(r, (bytes, bytearray)) else np.ascontiguousarray(r).tobytes(), dtype=np.uint8)
                if r.size > pitch:
                    raise DsmError(f"slot {b}'s frame has {r.size} bytes, the pitch is {pitch}")
                rows[b, :r.size] = r
            return rows
        rows = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        if rows.size != self.B * pitch:
            raise DsmError(f"raw rows: {rows.size} bytes, B x pitch is {self.B * pitch}")
        return np.ascontiguousarray(rows)

    def encode_step_raw(self, raw, mask, pitch=INGEST_MAX_FRAME_BYTES):
        rows = self._raw_rows(raw, pitch)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        codes = np.zeros((self.B, self.n_q), dtype=np.uint32)
        produced = C.c_int(0)
        self._check(self.lib.dsm_mimi_encode_step_raw(self.h, _ptr(rows), pitch, _ptr(mask), _ptr(codes), C.byref(produced)))
        return codes if produced.value else None

    def encode_step_raw_async(self, raw, mask, pitch=INGEST_MAX_FRAME_BYTES):
        rows = self._raw_rows(raw, pitch)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        ticket = C.c_int(-1)
        self._check(self.lib.dsm_mimi_encode_step_raw_async(self.h, _ptr(rows), pitch, _ptr(mask), C.byref(ticket)))
        return ticket.value

    def encode_step_raw_dev(self, d_raw, pitch, d_mask, d_codes):
        self._check(self.lib.dsm_mimi_encode_step_raw_dev(self.h, d_raw, pitch, d_mask, d_codes))

    def step_raw(self, raw, mask, pitch=INGEST_MAX_FRAME_BYTES):
        rows = self._raw_rows(raw, pitch)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        codes = np.zeros((self.B, self.n_q), dtype=np.uint32)
        text = np.zeros(self.B, dtype=np.uint32)
        nh = self.cfg.extra_heads_num
        prs = np.zeros((max(nh, 1), self.B), dtype=np.float32)
        self._check(self.lib.dsm_asr_step_raw(self.h, _ptr(rows), pitch, _ptr(mask), _ptr(codes), _ptr(text), _ptr(prs) if nh else None))
        return codes, text, prs[:nh]

    def debug_ingest_read(self, side=0):
        """The frames [B][1920] the side's (0 encoder, 1 model) last raw call handed to Mimi."""
        out = np.zeros((self.B, FRAME_SIZE), dtype=np.float32)
        self._check(self.lib.dsm_debug_ingest_read(self.h, int(side), _ptr(out)))
        return out

    # clips (include/dsm.h "clips"): a slot's audio resident on the device in its own format, K steps per visit
    def set_clips(self, on, max_clip_bytes=0):
        """dsm_asr_set_clips: the engine-wide switch; on allocates [B][max_clip_bytes] for the clips and turns ingest on."""
        self._check(self.lib.dsm_asr_set_clips(self.h, 1 if on else 0, int(max_clip_bytes)))

    def clip_begin(self, slot, rate, fmt=PCM_F32, flush_frames=0):
        """dsm_asr_clip_begin: the slot is reset on both sides, takes the format and has an empty open clip."""
        self._check(self.lib.dsm_asr_clip_begin(self.h, int(slot), int(rate), int(fmt), int(flush_frames)))

    def clip_push(self, slot, data):
        """dsm_asr_clip_push: appends bytes (any count) to the slot's clip."""
        data = bytes(data)
        buf = np.frombuffer(data, dtype=np.uint8) if data else None
        self._check(self.lib.dsm_asr_clip_push(self.h, int(slot), _ptr(buf), len(data)))

    def clip_close(self, slot):
        self._check(self.lib.dsm_asr_clip_close(self.h, int(slot)))

    def clip_status(self, slot):
        """ASR_CLIP_IDLE / RUNNING / WAITING / DONE."""
        return self._check(self.lib.dsm_asr_clip_status(self.h, int(slot)))

    def run(self, n_steps):
        """dsm_asr_run: enqueues n_steps (1..ASR_RUN_MAX) steps of every slot with a clip; nothing is read back until collect()."""
        self._check(self.lib.dsm_asr_run(self.h, int(n_steps)))

    def collect(self):
        """dsm_asr_collect: waits for the block.  Returns AsrBlock: stepped [n][B], text_token [n][B], vad_prs [n][heads][B],
        logprob [n][B], msgs — per step the list poll_msgs would give —, word_scores — per step [(batch_idx, logprobs)] of its
        Word messages —, status [B]."""
        n, B, nh = ASR_RUN_MAX, self.B, self.cfg.extra_heads_num
        stepped = np.zeros((n, B), dtype=np.uint8)
        text = np.zeros((n, B), dtype=np.uint32)
        prs = np.zeros((n, max(nh, 1), B), dtype=np.float32)
        lp = np.zeros((n, B), dtype=np.float32)
        status = np.zeros(B, dtype=np.int32)
        cap = n * (2 * B + 1)  # a step gives at most a Step, and a Word and an EndWord per slot
        msgs, step_of = (AsrMsg * cap)(), (C.c_int * cap)()
        toks, tlps = np.zeros(cap * 8, dtype=np.uint32), np.zeros(cap * 8, dtype=np.float32)
        blk = AsrBlockC(0, _ptr(stepped), _ptr(text), _ptr(prs) if nh else None, _ptr(lp), msgs, step_of, cap, 0, _ptr(toks),
                        _ptr(tlps), toks.size, 0, _ptr(status))
        self._check(self.lib.dsm_asr_collect(self.h, C.byref(blk)))
        k = blk.n_steps
        if blk.n_msgs > cap or blk.n_tokens > toks.size:
            raise DsmError(f"collect: {blk.n_msgs} messages / {blk.n_tokens} tokens do not fit the arrays")
        out, scores = [[] for _ in range(k)], [[] for _ in range(k)]
        for i in range(blk.n_msgs):
            m = msgs[i]
            if m.kind == MSG_WORD:
                out[step_of[i]].append(("Word", m.batch_idx, m.time, toks[m.tokens_offset:m.tokens_offset + m.n_tokens].tolist()))
                scores[step_of[i]].append((m.batch_idx, tlps[m.tokens_offset:m.tokens_offset + m.n_tokens].copy()))
            elif m.kind == MSG_END_WORD:
                out[step_of[i]].append(("EndWord", m.batch_idx, m.time))
            else:
                out[step_of[i]].append(("Step", m.step_idx))
        return AsrBlock(k, stepped[:k], text[:k], prs[:k, :nh], lp[:k], out, scores, status)

    # device-pointer variants (ints from torch.Tensor.data_ptr())
    def encode_step_dev(self, d_pcm, d_mask, d_codes):
        self._check(self.lib.dsm_mimi_encode_step_dev(self.h, d_pcm, d_mask, d_codes))

    def step_tokens_dev(self, d_codes, d_mask, d_text, d_prs):
        self._check(self.lib.dsm_asr_step_tokens_dev(self.h, d_codes, d_mask, d_text, d_prs))

    def streams_join(self):
        self._check(self.lib.dsm_streams_join(self.h))

    def step_pcm_dev(self, d_pcm, d_mask, d_codes=None, d_text=None, d_prs=None):
        self._check(self.lib.dsm_asr_step_pcm_dev(self.h, d_pcm, d_mask, d_codes, d_text, d_prs))

    def debug_set_positions(self, lm_pos, mimi_pos):
        self._check(self.lib.dsm_debug_set_positions(self.h, lm_pos, mimi_pos))

    def set_seed(self, slot, seed):
        """temperature > 0: restart the slot's Gumbel-noise stream (ChaCha12 keyed by seed_from_u64(seed))."""
        self._check(self.lib.dsm_asr_set_seed(self.h, slot, seed))

    def encode_step_async(self, pcm, mask):
        """dsm_mimi_encode_step_async: enqueue the frame's encode, return its ticket for step_tokens_ticket."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(self.B, FRAME_SIZE)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        ticket = C.c_int(-1)
        self._check(self.lib.dsm_mimi_encode_step_async(self.h, _ptr(pcm), _ptr(mask), C.byref(ticket)))
        return ticket.value

    def step_tokens_ticket(self, ticket, mask):
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        text = np.zeros(self.B, dtype=np.uint32)
        nh = self.cfg.extra_heads_num
        prs = np.zeros((max(nh, 1), self.B), dtype=np.float32)
        self._check(self.lib.dsm_asr_step_tokens_ticket(self.h, ticket, _ptr(mask), _ptr(text), _ptr(prs) if nh else None))
        return text, prs[:nh]

    # slot snapshots (include/dsm.h "slot snapshots"; INTEGRATION.md has the drain / compact / resume recipes)
    @staticmethod
    def _slot_list(slots):
        slots = [int(s) for s in slots]
        return (C.c_int * max(len(slots), 1))(*slots), len(slots)

    def export_slots(self, slots):
        """The listed slots' whole stream state as one blob (bytes).  The slots themselves are left as they are: reset them
        (reset_batch_idx + mimi_reset_batch_idx) before another stream takes them."""
        arr, n = self._slot_list(slots)
        need = C.c_size_t(0)
        self._check(self.lib.dsm_asr_export_slots(self.h, arr, n, None, 0, C.byref(need)))
        buf = bytearray(need.value)  # a blob is ~100 MB per slot at the served presets: the library writes into it in place
        self._check(self.lib.dsm_asr_export_slots(self.h, arr, n, (C.c_char * need.value).from_buffer(buf), need.value, C.byref(need)))
        return bytes(buf)

    def import_slots(self, slots, blob):
        """Slot i of `blob` (export_slots of an engine of the same configuration; batch size and device may differ) into
        slots[i].  DsmError, engine unchanged, when the blob does not fit."""
        arr, n = self._slot_list(slots)
        blob = bytes(blob)
        self._check(self.lib.dsm_asr_import_slots(self.h, arr, n, blob, len(blob)))

    def move_slots(self, src_slots, dst, dst_slots):
        """This engine's src_slots[i] -> dst's dst_slots[i], device to device (same device only); dst may be self (a fork)."""
        sa, n = self._slot_list(src_slots)
        da, nd = self._slot_list(dst_slots)
        if n != nd:
            raise DsmError("move_slots: the two slot lists differ in length")
        self._check(self.lib.dsm_asr_move_slots(self.h, sa, dst.h, da, n))

    def debug_set_text_tokens(self, tokens):
        """Teacher forcing: the text token every slot feeds back into its next step."""
        t = np.ascontiguousarray(tokens, dtype=np.uint32)
        assert t.shape == (self.B,)
        self._check(self.lib.dsm_debug_set_text_tokens(self.h, t.ctypes.data))

    def debug_gemm(self, M, N, K, X, xmap, W, bf16, epi=EPI_STORE, bias=None, scale=None, act=0, res=None, rmap=None,
                   Y=None, ymap=None, Y2=None, y2map=None, norm_w=None, norm_b=None, norm_out=None, may_defer=False,
                   knobs=(-1, -1, -1, -1, -1)):
        """dsm_debug_gemm, a test aid: one product through the engine's GEMM launcher.  X, res, Y, Y2 and norm_out are flat
        float32 buffers, each with its row map (bstride, rpb, ld, toff); Y, Y2 and norm_out hold what the caller wants to find
        again outside the M x N result.  W is [N][K] ([2 N][K] for the gate).  norm_b None with norm_w: RmsNorm.  Returns a dict:
        plan (the line of the plan that ran), Y / Y2 / norm_out (the whole buffers afterwards, copies), x_back / res_back (the
        device copies of X / res afterwards) and w_changed."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1)  # noqa: E731
        X, W, bias, scale, res, norm_w, norm_b = (f32(a) for a in (X, W, bias, scale, res, norm_w, norm_b))
        out = {k: (None if a is None else f32(a).copy()) for k, a in (("Y", Y), ("Y2", Y2), ("norm_out", norm_out))}
        assert W.size == (2 * N if epi == EPI_GATE else N) * K, "W is [N][K] (the gate: [2 N][K])"
        for name, a in (("bias", bias), ("scale", scale), ("norm_w", norm_w), ("norm_b", norm_b)):
            assert a is None or a.size == N, name + " is [N]"
        g = DebugGemmArgs()
        g.M, g.N, g.K, g.weight_bf16, g.epi, g.act, g.may_defer = M, N, K, int(bool(bf16)), epi, act, int(bool(may_defer))
        g.norm_rms = int(norm_w is not None and norm_b is None)
        g.knobs = (C.c_int32 * 5)(*knobs)
        back = {"x_back": np.zeros_like(X), "res_back": None if res is None else np.zeros_like(res)}
        g.X, g.x_len, g.xmap, g.W = X.ctypes.data, X.size, DebugRowMap(*xmap), W.ctypes.data
        g.bias, g.scale = _ptr(bias), _ptr(scale)
        if res is not None:
            g.res, g.res_len, g.rmap, g.res_back = res.ctypes.data, res.size, DebugRowMap(*rmap), back["res_back"].ctypes.data
        if out["Y"] is not None:
            g.Y, g.y_len, g.ymap = out["Y"].ctypes.data, out["Y"].size, DebugRowMap(*ymap)
        if out["Y2"] is not None:
            g.Y2, g.y2_len, g.y2map = out["Y2"].ctypes.data, out["Y2"].size, DebugRowMap(*y2map)
        if out["norm_out"] is not None:
            g.norm_w, g.norm_b, g.norm_out, g.norm_len = _ptr(norm_w), _ptr(norm_b), out["norm_out"].ctypes.data, out["norm_out"].size
        g.x_back = back["x_back"].ctypes.data
        plan = C.create_string_buffer(512)
        self._check(self.lib.dsm_debug_gemm(self.h, C.byref(g), plan, len(plan)))
        return dict(out, plan=plan.value.decode(), w_changed=bool(g.w_changed), **back)

    def prof_read_device(self):
        """Like prof_read, from the in-kernel device-clock brackets (attention classes only)."""
        tot = (C.c_double * len(PROF_TAGS))()
        cnt = (C.c_uint64 * len(PROF_TAGS))()
        self._check(self.lib.dsm_prof_read_device(self.h, tot, cnt))
        return {t: (tot[i], cnt[i]) for i, t in enumerate(PROF_TAGS)}

    def prof_timeline(self, on):
        self._check(self.lib.dsm_prof_timeline(self.h, 1 if on else 0))

    def prof_timeline_read(self, cap=1 << 16):
        """[(stream id, kind, tag name, start_us, end_us), ...] of every bracketed launch since the last read."""
        sid, kind, tag = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        t0, t1 = (C.c_double * cap)(), (C.c_double * cap)()
        n = self._check(self.lib.dsm_prof_timeline_read(self.h, sid, kind, tag, t0, t1, cap))
        return [(sid[i], kind[i], PROF_TAGS[tag[i]], t0[i], t1[i]) for i in range(n)]

    def stream_groups(self):
        """[(first_slot, n_slots), ...] of the LM stream groups."""
        a, b = (C.c_int * 8)(), (C.c_int * 8)()
        g = self._check(self.lib.dsm_lm_stream_groups(self.h, a, b, 8))
        return [(a[i], b[i]) for i in range(g)]

    def debug_serialize_groups(self, on):
        self._check(self.lib.dsm_debug_serialize_groups(self.h, 1 if on else 0))

    def prof_enable(self, tags):
        mask = 0
        for t in tags:
            mask |= 1 << PROF_TAGS.index(t)
        self._check(self.lib.dsm_prof_enable(self.h, mask))

    def prof_read(self):
        tot = (C.c_double * len(PROF_TAGS))()
        cnt = (C.c_uint64 * len(PROF_TAGS))()
        self._check(self.lib.dsm_prof_read(self.h, tot, cnt))
        return {t: (tot[i], cnt[i]) for i, t in enumerate(PROF_TAGS)}


class TtsEngine:
    """B independent tts_streaming::State generations behind the C ABI (core/tts_streaming.rs:117-242).
    step() mirrors State::step(prev_text_token, allowed_tokens, conditions=None) with greedy sampling."""

    def __init__(self, cfg, batch_size, lm_path, device_id=0):
        self.lib = load_library()
        self.cfg, self.B, self.S = cfg, batch_size, cfg.dep_num_slices
        self.n_speakers = 0  # set by attach_speaker_encoder
        h = C.c_void_p()
        rc = self.lib.dsm_tts_create(C.byref(cfg), device_id, batch_size, lm_path.encode(), C.byref(h))
        if rc != 0:
            msg = self.lib.dsm_tts_last_error(None)
            raise DsmError(f"dsm_tts_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.h = h

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.dsm_tts_last_error(self.h)
            raise DsmError(f"dsm error {rc}: {msg.decode() if msg else '?'}")
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.dsm_tts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, prev_text_token, allowed, mask):
        prev = np.ascontiguousarray(prev_text_token, dtype=np.uint32).reshape(self.B)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32).reshape(self.B)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        text = np.zeros(self.B, dtype=np.uint32)
        audio = np.zeros((self.B, self.S), dtype=np.uint32)
        self._check(self.lib.dsm_tts_step(self.h, _ptr(prev), _ptr(allowed), _ptr(mask), _ptr(text), _ptr(audio)))
        return text, audio

    def attach_mimi(self, mimi_cfg, path):
        """The Mimi that decodes the generated frames (srv/tts.rs:309-310); needs n_q == dep_num_slices."""
        self._check(self.lib.dsm_tts_attach_mimi(self.h, C.byref(mimi_cfg), path.encode()))

    def step_pcm(self, prev_text_token, allowed, mask, defer=False):
        """step() + the decode of the frame the step completed.  Returns (text, audio, pcm [B][1920], valid [B]); with
        defer=True only (text, audio): the decode is enqueued and its result comes out of recv_pcm(), in order."""
        prev = np.ascontiguousarray(prev_text_token, dtype=np.uint32).reshape(self.B)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32).reshape(self.B)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        text = np.zeros(self.B, dtype=np.uint32)
        audio = np.zeros((self.B, self.S), dtype=np.uint32)
        pcm = None if defer else np.zeros((self.B, FRAME_SIZE), dtype=np.float32)
        valid = None if defer else np.zeros(self.B, dtype=np.uint8)
        self._check(self.lib.dsm_tts_step_pcm(self.h, _ptr(prev), _ptr(allowed), _ptr(mask), _ptr(text), _ptr(audio),
                                              _ptr(pcm), _ptr(valid)))
        return (text, audio) if defer else (text, audio, pcm, valid)

    def recv_pcm(self):
        """The oldest deferred step's (pcm, valid), or None when nothing is pending."""
        pcm = np.zeros((self.B, FRAME_SIZE), dtype=np.float32)
        valid = np.zeros(self.B, dtype=np.uint8)
        if self._check(self.lib.dsm_tts_recv_pcm(self.h, _ptr(pcm), _ptr(valid))) == 0:
            return None
        return pcm, valid

    def pcm_pending(self):
        return self._check(self.lib.dsm_tts_pcm_pending(self.h))

    # egress (include/dsm.h "egress"): per-slot output sample rate and sample format, resampled and encoded on the device
    def set_egress(self, on):
        """dsm_tts_set_egress: the engine-wide switch; on allocates the section, and decodes then deliver raw rows only."""
        self._check(self.lib.dsm_tts_set_egress(self.h, 1 if on else 0))

    def set_output_format(self, slot, rate, fmt=PCM_F32):
        """dsm_tts_set_output_format: the slot's format from its next emitted frame on; clears its history."""
        self._check(self.lib.dsm_tts_set_output_format(self.h, int(slot), int(rate), int(fmt)))

    def output_format(self, slot):
        """(rate, fmt, frame_samples, frame_bytes, latency in output samples) of the slot."""
        v = [C.c_int(0) for _ in range(5)]
        self._check(self.lib.dsm_tts_output_format(self.h, int(slot), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def step_raw(self, prev_text_token, allowed, mask, defer=False, pitch=EGRESS_MAX_FRAME_BYTES, fill=0):
        """step_pcm's raw sibling.  Returns (text, audio, rows [B][pitch] uint8, valid [B]): slot b's frame is the first
        frame_bytes(b) bytes of its row, everything else keeps `fill`.  defer=True: (text, audio), rows through recv_raw()."""
        prev = np.ascontiguousarray(prev_text_token, dtype=np.uint32).reshape(self.B)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32).reshape(self.B)
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        text = np.zeros(self.B, dtype=np.uint32)
        audio = np.zeros((self.B, self.S), dtype=np.uint32)
        rows = None if defer else np.full((self.B, pitch), fill, dtype=np.uint8)
        valid = None if defer else np.zeros(self.B, dtype=np.uint8)
        self._check(self.lib.dsm_tts_step_raw(self.h, _ptr(prev), _ptr(allowed), _ptr(mask), _ptr(text), _ptr(audio),
                                              _ptr(rows), pitch, _ptr(valid)))
        return (text, audio) if defer else (text, audio, rows, valid)

    def recv_raw(self, pitch=EGRESS_MAX_FRAME_BYTES, fill=0):
        """The oldest deferred step's (rows [B][pitch], valid), or None when nothing is pending."""
        rows = np.full((self.B, pitch), fill, dtype=np.uint8)
        valid = np.zeros(self.B, dtype=np.uint8)
        if self._check(self.lib.dsm_tts_recv_raw(self.h, _ptr(rows), pitch, _ptr(valid))) == 0:
            return None
        return rows, valid

    def debug_egress(self, pcm, valid, pitch=EGRESS_MAX_FRAME_BYTES, fill=0):
        """dsm_tts_debug_egress: the kernel alone on frames [B][1920] and valid flags [B]; rows [B][pitch] uint8."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(self.B, FRAME_SIZE)
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(self.B)
        rows = np.full((self.B, pitch), fill, dtype=np.uint8)
        self._check(self.lib.dsm_tts_debug_egress(self.h, _ptr(pcm), _ptr(valid), _ptr(rows), pitch))
        return rows

    def audio_tokens(self, slot, step):
        out = np.zeros(self.S, dtype=np.uint32)
        self._check(self.lib.dsm_tts_audio_tokens(self.h, slot, step, _ptr(out)))
        return out

    def step_idx(self, slot):
        return self._check(self.lib.dsm_tts_step_idx(self.h, slot))

    def reset_batch_idx(self, slot):
        self._check(self.lib.dsm_tts_reset_slot(self.h, slot))

    def debug_read(self, name, n):
        out = np.zeros(n, dtype=np.float32)
        got = self._check(self.lib.dsm_tts_debug_read(self.h, name.encode(), _ptr(out), n))
        return out[:got]

    def metrics(self):
        m = Metrics()
        self._check(self.lib.dsm_tts_get_metrics(self.h, C.byref(m)))
        return m

    def set_sampling(self, slot, top_k, temperature, seed):
        """Sampling::TopK{k, temperature} seeded with `seed` for the slot's text and audio processors (srv/tts.rs:401-415)."""
        self._check(self.lib.dsm_tts_set_sampling(self.h, slot, top_k, temperature, seed))

    def attach_speaker_encoder(self, n_speakers, lm_path):
        """SpeakerEncoder::new on the attached Mimi (core/tts_streaming.rs:346-372): output_proj and learnt_padding from lm_path."""
        self._check(self.lib.dsm_tts_attach_speaker_encoder(self.h, n_speakers, lm_path.encode()))
        self.n_speakers = n_speakers

    def encode_voice(self, clips):
        """SpeakerEncoder::encode: clips [n_clips][clip_len] f32 at 24 kHz -> ca_src rows [n_speakers * clip_len / 1920][cond_dim]."""
        a = np.ascontiguousarray(clips, dtype=np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        cond = self.cfg.ca_dim or self.cfg.lm.d_model
        cap = max(1, self.n_speakers * (a.shape[1] // FRAME_SIZE))
        out, rows = np.zeros((cap, cond), dtype=np.float32), C.c_int(0)
        self._check(self.lib.dsm_tts_encode_voice(self.h, _ptr(a), a.shape[0], a.shape[1], _ptr(out), cap, C.byref(rows)))
        return out[:rows.value]

    def speaker_empty(self):
        """SpeakerEncoder::empty: the unconditional source of a guided request, [n_speakers * 125][cond_dim]."""
        cond = self.cfg.ca_dim or self.cfg.lm.d_model
        cap = max(1, self.n_speakers * 125)
        out, rows = np.zeros((cap, cond), dtype=np.float32), C.c_int(0)
        self._check(self.lib.dsm_tts_speaker_empty(self.h, _ptr(out), cap, C.byref(rows)))
        return out[:rows.value]

    # ---- a request's text schedule on the device (srv/tts.rs:574-621), K steps per visit ----
    def request_begin(self, slot, max_seq_len, extra_steps=0):
        """Starts a request on a fresh slot (reset_batch_idx, then set_ca_src / set_sampling as needed)."""
        self._check(self.lib.dsm_tts_request_begin(self.h, slot, max_seq_len, extra_steps))

    def push_words(self, slot, words):
        """in_tx.send(Some(word_tokens)) for each word: a list of token lists (a word may be empty); the caller puts the
        bos token in front of the first word's tokens (srv/tts.rs:484-493)."""
        lens = np.array([len(w) for w in words], dtype=np.int32)
        toks = np.array([t for w in words for t in w], dtype=np.uint32)
        self._check(self.lib.dsm_tts_request_push_words(self.h, slot, _ptr(toks) if toks.size else None, _ptr(lens), len(words)))

    def attach_tokenizer(self, path):
        """The SentencePiece model of push_text / word_text (the server's text_tokenizer); once per engine."""
        self._check(self.lib.dsm_tts_attach_tokenizer(self.h, os.fsencode(path)))

    def push_text(self, slot, text):
        """One text message of the client (srv/tts.rs:480-494): split on spaces, each word encoded on its own, the bos in
        front of the request's first word.  Returns the number of words queued; all or nothing."""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        n = C.c_int(0)
        self._check(self.lib.dsm_tts_request_push_text(self.h, slot, raw, len(raw), C.byref(n)))
        return n.value

    def word_text(self, slot, word):
        """WordWithTimestamps.text of word event `word` (-1: the initial empty word), as bytes."""
        n = self._check(self.lib.dsm_tts_word_text(self.h, slot, word, None, 0))
        out = C.create_string_buffer(max(1, n))
        self._check(self.lib.dsm_tts_word_text(self.h, slot, word, out, n))
        return out.raw[:n]

    def request_close(self, slot):
        """in_tx.send(None): no more words."""
        self._check(self.lib.dsm_tts_request_close(self.h, slot))

    def run(self, n_steps, decode=False):
        """Enqueues n_steps (1..TTS_RUN_MAX) steps of every slot with a request; nothing is read back until collect()."""
        self._check(self.lib.dsm_tts_run(self.h, n_steps, 1 if decode else 0))
        self._run = (n_steps, bool(decode))

    def collect(self):
        """Waits for the block.  Returns TtsBlock: stepped [n][B], text_token [n][B], audio [n][B][S], pcm [n][B][1920] and
        pcm_valid [n][B] (None unless run(decode=True)), events [(slot, word, start_step, stop_step)], status [B]."""
        n, decode = getattr(self, "_run", None) or (TTS_RUN_MAX, False)
        B = self.B
        stepped = np.zeros((n, B), dtype=np.uint8)
        text = np.zeros((n, B), dtype=np.uint32)
        audio = np.zeros((n, B, self.S), dtype=np.uint32)
        pcm = np.zeros((n, B, FRAME_SIZE), dtype=np.float32) if decode else None
        valid = np.zeros((n, B), dtype=np.uint8) if decode else None
        status = np.zeros(B, dtype=np.int32)
        ev = (TtsWordEvent * (n * B))()
        blk = TtsBlockC(0, _ptr(stepped), _ptr(text), _ptr(audio), _ptr(pcm), _ptr(valid), ev, n * B, 0, _ptr(status))
        self._check(self.lib.dsm_tts_collect(self.h, C.byref(blk)))
        self._run = None
        k = blk.n_steps
        events = [(e.slot, e.word, e.start_step, e.stop_step) for e in ev[:blk.n_events]]
        return TtsBlock(k, stepped[:k], text[:k], audio[:k], None if pcm is None else pcm[:k],
                        None if valid is None else valid[:k], events, status)

    def collect_raw(self, pitch=EGRESS_MAX_FRAME_BYTES, fill=0):
        """collect()'s raw sibling (egress on): the TtsBlock's pcm is the raw rows [n][B][pitch] uint8 — slot b's frame of step
        s in the first frame_bytes(b) bytes of its row, everything else keeps `fill` (None unless run(decode=True))."""
        n, decode = getattr(self, "_run", None) or (TTS_RUN_MAX, False)
        B = self.B
        stepped = np.zeros((n, B), dtype=np.uint8)
        text = np.zeros((n, B), dtype=np.uint32)
        audio = np.zeros((n, B, self.S), dtype=np.uint32)
        rows = np.full((n, B, pitch), fill, dtype=np.uint8) if decode else None
        valid = np.zeros((n, B), dtype=np.uint8) if decode else None
        status = np.zeros(B, dtype=np.int32)
        ev = (TtsWordEvent * (n * B))()
        blk = TtsBlockC(0, _ptr(stepped), _ptr(text), _ptr(audio), None, _ptr(valid), ev, n * B, 0, _ptr(status))
        self._check(self.lib.dsm_tts_collect_raw(self.h, C.byref(blk), _ptr(rows), pitch))
        self._run = None
        k = blk.n_steps
        events = [(e.slot, e.word, e.start_step, e.stop_step) for e in ev[:blk.n_events]]
        return TtsBlock(k, stepped[:k], text[:k], audio[:k], None if rows is None else rows[:k],
                        None if valid is None else valid[:k], events, status)

    def request_status(self, slot):
        return self._check(self.lib.dsm_tts_request_status(self.h, slot))

    def set_ca_src(self, slot, ca_src, ca_src_uncond=None, cfg_alpha=0.0):
        """State::new's ca_src / cfg_alpha for the slot (srv/tts.rs:426-441): ca_src [n][ca_dim] f32 or None;
        ca_src_uncond: the second batch row of a classifier-free-guidance request."""
        a = None if ca_src is None else np.ascontiguousarray(ca_src, dtype=np.float32)
        u = None if ca_src_uncond is None else np.ascontiguousarray(ca_src_uncond, dtype=np.float32)
        self._check(self.lib.dsm_tts_set_ca_src(self.h, slot, _ptr(a), 0 if a is None else a.shape[0], _ptr(u),
                                                0 if u is None else u.shape[0], float(cfg_alpha)))

    # ---- voices: a source projected once on the device, shared by the slots that attach to it ----
    def voice_create(self, rows):
        """ca_src rows [n][cond_dim] f32 -> a voice handle (> 0): the in_proj_kv projection of every layer, kept on the device."""
        a = np.ascontiguousarray(rows, dtype=np.float32)
        n = a.shape[0] if a.ndim == 2 else 0
        v = C.c_int(0)
        self._check(self.lib.dsm_tts_voice_create(self.h, _ptr(a) if n and a.size else None, n, C.byref(v)))
        return v.value

    def voice_destroy(self, voice):
        self._check(self.lib.dsm_tts_voice_destroy(self.h, voice))

    def voice_info(self, voice):
        """(rows, batch rows attached, device bytes)"""
        rows, refs, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0)
        self._check(self.lib.dsm_tts_voice_info(self.h, voice, C.byref(rows), C.byref(refs), C.byref(nbytes)))
        return rows.value, refs.value, nbytes.value

    def set_voice(self, slot, voice, uncond=0, cfg_alpha=0.0):
        """set_ca_src by reference: the slot's rows read `voice` (and `uncond`, the second batch row of a guided request)."""
        self._check(self.lib.dsm_tts_set_voice(self.h, slot, voice, uncond, float(cfg_alpha)))

    def voice_from_clips(self, clips):
        """encode_voice, then voice_create."""
        return self.voice_create(self.encode_voice(clips))

    def voice_empty(self):
        """speaker_empty, then voice_create: the unconditional voice every guided request shares."""
        return self.voice_create(self.speaker_empty())

    # ---- conditioners (core/conditioner.rs): one Condition::AddToInput per slot ----
    def attach_conditioners(self, descs, lm_path):
        """ConditionProvider::new: descs as config_toml.load_tts_conditioners returns them — dicts with name, type ("Lut" /
        "ContinuousAttribute"), dim and n_bins + possible_values or scale_factor + max_period; tensors from lm_path."""
        arr = (TtsConditionerDesc * len(descs))()
        keep = []  # the strings the array points to
        for a, dsc in zip(arr, descs):
            if dsc["type"] not in ("Lut", "ContinuousAttribute"):
                raise ValueError(f"conditioner type {dsc['type']!r}")
            name = dsc["name"].encode()
            keep.append(name)
            a.name, a.dim = name, int(dsc["dim"])
            if dsc["type"] == "Lut":
                vals = (C.c_char_p * len(dsc["possible_values"]))(*[v.encode() for v in dsc["possible_values"]])
                keep.append(vals)
                a.type, a.n_bins, a.possible_values, a.n_values = TTS_COND_LUT, int(dsc["n_bins"]), vals, len(vals)
            else:
                a.type, a.scale_factor, a.max_period = TTS_COND_CONTINUOUS, float(dsc["scale_factor"]), float(dsc["max_period"])
        self._check(self.lib.dsm_tts_attach_conditioners(self.h, arr, len(descs), lm_path.encode()))

    def set_condition(self, slot, name, value):
        """condition_lut (value: str) or condition_cont (value: a number) on a fresh slot; replaces the slot's condition."""
        if isinstance(value, str):
            self._check(self.lib.dsm_tts_set_condition_lut(self.h, slot, name.encode(), value.encode()))
        else:
            self._check(self.lib.dsm_tts_set_condition_cont(self.h, slot, name.encode(), float(value)))

    def set_condition_padding(self, slot, name):
        """The conditioner's learnt_padding as the slot's condition."""
        self._check(self.lib.dsm_tts_set_condition_padding(self.h, slot, name.encode()))

    def clear_condition(self, slot):
        self._check(self.lib.dsm_tts_clear_condition(self.h, slot))
