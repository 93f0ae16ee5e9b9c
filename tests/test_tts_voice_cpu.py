"""The voice calls of the C ABI without a GPU: the four symbols are exported with the signatures include/dsm.h declares, each
refuses a NULL engine with DSM_ERR_INVALID, and TtsEngine carries the wrappers.  What they compute: tests/test_tts_voice_gpu.py."""
import ctypes as C
import inspect
import os
import re

DSM_ERR_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "dsm_tts_voice_create": "int dsm_tts_voice_create(dsm_tts*, const float* ca_src, int n, int* voice_out);",
    "dsm_tts_voice_destroy": "int dsm_tts_voice_destroy(dsm_tts*, int voice);",
    "dsm_tts_voice_info": "int dsm_tts_voice_info(dsm_tts*, int voice, int* rows, int* refs, size_t* device_bytes);",
    "dsm_tts_set_voice": "int dsm_tts_set_voice(dsm_tts*, int slot, int voice, int voice_uncond, double cfg_alpha);",
}


def test_the_header_declares_the_four_calls_as_specified():
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).replace(" ,", ",")
    for name, decl in DECLARED.items():
        assert decl in hdr, f"{name}: include/dsm.h does not declare `{decl}`"


def test_symbols_are_exported_with_those_signatures_and_refuse_a_null_engine(dsm, lib):
    ip, zp = C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    want = {
        "dsm_tts_voice_create": [C.c_void_p, C.c_void_p, C.c_int, ip],
        "dsm_tts_voice_destroy": [C.c_void_p, C.c_int],
        "dsm_tts_voice_info": [C.c_void_p, C.c_int, ip, ip, zp],
        "dsm_tts_set_voice": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double],
    }
    for name, argtypes in want.items():
        assert name in dsm.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int, name
    rows = (C.c_float * 8)()
    v, a, b, n = C.c_int(7), C.c_int(7), C.c_int(7), C.c_size_t(7)
    assert lib.dsm_tts_voice_create(None, rows, 1, C.byref(v)) == DSM_ERR_INVALID
    assert lib.dsm_tts_voice_destroy(None, 1) == DSM_ERR_INVALID
    assert lib.dsm_tts_voice_info(None, 1, C.byref(a), C.byref(b), C.byref(n)) == DSM_ERR_INVALID
    assert lib.dsm_tts_set_voice(None, 0, 1, 0, 0.0) == DSM_ERR_INVALID
    assert (a.value, b.value, n.value) == (7, 7, 7)  # nothing written on a refusal


def test_the_python_wrappers_exist(dsm):
    params = {
        "voice_create": ["rows"], "voice_destroy": ["voice"], "voice_info": ["voice"],
        "set_voice": ["slot", "voice", "uncond", "cfg_alpha"], "voice_from_clips": ["clips"], "voice_empty": [],
    }
    for name, want in params.items():
        fn = getattr(dsm.TtsEngine, name, None)
        assert callable(fn), f"TtsEngine.{name} is missing"
        assert list(inspect.signature(fn).parameters)[1:] == want, name
    sig = inspect.signature(dsm.TtsEngine.set_voice).parameters
    assert sig["uncond"].default == 0 and sig["cfg_alpha"].default == 0.0
