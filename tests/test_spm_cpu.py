"""The native SentencePiece tokenizer (csrc/dsm_spm.h behind dsm_spm_*) against Python `sentencepiece`: the vectors recorded
from the module in tests/golden/spm/vectors.json (always), the module itself on seeded random input (where it is installed),
the refusals, and the STT worker's Word.text on the oracle backend.  Byte-identical everywhere: there is no tolerance in this
feature.  The TTS refusals that need an engine (push_text / word_text without a tokenizer, a tokenizer larger than the TTS
vocabulary) are in test_spm_gpu.py: a dsm_tts exists only on a device."""
import ctypes as C
import os
import random

import pytest

import spm_ref
import worker_ref
from test_worker_cpu import run_script

DSM_ERR_INVALID, DSM_ERR_IO, DSM_ERR_STATE = -1, -2, -4
MODELS = ["uni512_nfkc_bf", "uni64", "uni40"]


def model_path(name):
    return os.path.join(spm_ref.GOLDEN, name + ".model")


def module(name):
    try:
        import sentencepiece
    except ImportError:
        pytest.skip("Python sentencepiece is not installed")
    return sentencepiece.SentencePieceProcessor(model_file=model_path(name))


@pytest.mark.parametrize("name", MODELS)
def test_recorded_vectors(dsm, lib, name):
    rec = spm_ref.vectors()["models"][name]
    assert len(rec["encode"]) >= 200 and len(rec["decode"]) >= 200
    with open(model_path(name), "rb") as f:
        from_bytes = dsm.Tokenizer(f.read())
    for tok in (dsm.Tokenizer(model_path(name)), from_bytes):
        assert tok.vocab_size == len(rec["pieces"])
        assert list(tok.special_ids) == rec["special_ids"]
        for text_hex, ids in rec["encode"]:
            assert tok.encode(bytes.fromhex(text_hex)) == ids, bytes.fromhex(text_hex)
        for ids, text_hex in rec["decode"]:
            assert tok.decode(ids) == bytes.fromhex(text_hex), ids
        tok.close()


def test_size_convention(dsm, lib):
    """A buffer that is too small gets the needed count and not one byte."""
    import numpy as np
    tok = dsm.Tokenizer(model_path("uni64"))
    text = b"the engine decodes frames"
    want = tok.encode(text)
    ids = np.full(len(want), 0xdeadbeef, dtype=np.uint32)
    assert lib.dsm_spm_encode(tok.h, text, len(text), ids.ctypes.data_as(C.c_void_p), len(want) - 1) == len(want)
    assert (ids == 0xdeadbeef).all()
    assert lib.dsm_spm_encode(tok.h, text, len(text), ids.ctypes.data_as(C.c_void_p), len(want)) == len(want) and list(ids) == want
    back = tok.decode(want)
    buf = C.create_string_buffer(b"\x55" * len(back), len(back))
    assert lib.dsm_spm_decode(tok.h, ids.ctypes.data_as(C.c_void_p), ids.size, buf, len(back) - 1) == len(back)
    assert buf.raw == b"\x55" * len(back)
    assert lib.dsm_spm_decode(tok.h, ids.ctypes.data_as(C.c_void_p), ids.size, buf, len(back)) == len(back) and buf.raw == back
    tok.close()


def random_texts(sp, rng, n):
    """Strings of the model's own pieces, random Unicode scalars and random bytes (malformed UTF-8 and NUL included)."""
    pieces = [sp.id_to_piece(i) for i in range(sp.get_piece_size())]
    for _ in range(n):
        kind = rng.randrange(4)
        if kind == 0:
            yield "".join(rng.choice(pieces).replace("▁", " ") for _ in range(rng.randrange(0, 10))).encode()
        elif kind == 1:
            yield "".join(chr(rng.choice([rng.randrange(0x20, 0x7f), 0x20, rng.randrange(0xa0, 0x3000), rng.randrange(0xff00, 0xfff0),
                                          rng.randrange(0x10000, 0x20000), rng.randrange(0, 0x20), rng.randrange(0xe000, 0x110000)]))
                          for _ in range(rng.randrange(0, 20))).encode()
        elif kind == 2:
            yield bytes(rng.randrange(256) for _ in range(rng.randrange(0, 20)))
        else:
            yield "".join(rng.choice("abcdefghij   eé①Ａ▁") for _ in range(rng.randrange(0, 30))).encode()


def random_id_runs(vocab, rng, n):
    for _ in range(n):
        yield [rng.randrange(vocab) if rng.random() < 0.7 else rng.choice([0, 1, 2, 3]) for _ in range(rng.randrange(0, 10))]


@pytest.mark.parametrize("name", MODELS)
def test_live_comparison_with_the_module(dsm, lib, name):
    sp = module(name)
    tok = dsm.Tokenizer(model_path(name))
    rng = random.Random("live-" + name)
    for text in random_texts(sp, rng, 2000):
        assert tok.encode(text) == sp.encode(text), text
    for ids in random_id_runs(sp.get_piece_size(), rng, 2000):
        assert tok.decode(ids) == sp.decode(ids).encode("utf-8"), ids
    assert list(tok.special_ids) == [sp.unk_id(), sp.bos_id(), sp.eos_id(), sp.pad_id()]
    tok.close()


@pytest.mark.parametrize("name", MODELS)
def test_spm_ref_decode_is_the_modules(name):
    sp = module(name)
    rng = random.Random("ref-" + name)
    for ids in random_id_runs(sp.get_piece_size(), rng, 2000):
        assert spm_ref.decode(name, ids) == sp.decode(ids).encode("utf-8"), ids
    for ids, text_hex in spm_ref.vectors()["models"][name]["decode"]:
        assert spm_ref.decode(name, ids) == bytes.fromhex(text_hex)


def load_fails(dsm, model):
    with pytest.raises(dsm.DsmError) as ei:
        dsm.Tokenizer(model)
    message = str(ei.value).split(": ", 1)[1]
    assert message.strip(), "a refusal carries a message"
    return ei.value.code, message


def test_refused_models(dsm, lib):
    assert spm_ref.vectors()["refused"] == ["bpe64.model"]
    code, message = load_fails(dsm, model_path("bpe64"))
    assert code == DSM_ERR_INVALID and "BPE" in message
    code, message = load_fails(dsm, os.path.join(spm_ref.GOLDEN, "no_such.model"))
    assert code == DSM_ERR_IO
    code, message = load_fails(dsm, b"")
    assert code == DSM_ERR_IO


@pytest.mark.parametrize("name", MODELS)
def test_truncated_files_are_refused(dsm, lib, name):
    with open(model_path(name), "rb") as f:
        blob = f.read()
    rng = random.Random("cut-" + name)
    for cut in [rng.randrange(len(blob)) for _ in range(64)]:
        code, message = load_fails(dsm, blob[:cut])
        assert code == DSM_ERR_IO, (cut, message)


def test_id_beyond_the_vocabulary_is_an_error(dsm, lib):
    tok = dsm.Tokenizer(model_path("uni40"))
    for ids in ([40], [5, 6, 40, 7], [0xffffffff]):
        with pytest.raises(dsm.DsmError) as ei:
            tok.decode(ids)
        assert ei.value.code == DSM_ERR_INVALID and "out of range" in str(ei.value)
    assert tok.decode([5, 6, 39, 7])  # the last id of the model is fine
    tok.close()


def test_tokenizer_larger_than_the_backend_vocabulary(dsm, lib, orc, tiny_weights):
    cfg = dsm.config_tiny()
    be, keep = worker_ref.oracle_backend(dsm, orc.OracleAsr(cfg, 2, *tiny_weights), cfg, 2)
    be.text_out_vocab_size = 40
    w = dsm.Worker(backend=be)
    with pytest.raises(dsm.DsmError, match="64 pieces") as ei:
        w.set_tokenizer_file(model_path("uni64"))
    assert ei.value.code == DSM_ERR_INVALID
    w.set_tokenizer_file(model_path("uni40"))  # one that fits is taken
    with pytest.raises(dsm.DsmError, match="BPE") as ei:
        w.set_tokenizer_file(model_path("bpe64"))
    assert ei.value.code == DSM_ERR_INVALID
    w.close()


WORKER_SEED = 3  # worker_ref.script's seed: this run delivers Words that carry tokens (asserted below)


def test_worker_word_text_on_the_oracle(dsm, lib, orc, tiny_weights):
    """tokenizer_file = uni64.model (config_tiny's text vocabulary is 64): message for message what RefWorker delivers with
    spm_ref.decode; a callback beside the file wins; with neither the decimal ids stay."""
    cfg = dsm.config_tiny()
    B = 4
    events = worker_ref.script(B, 40, seed=WORKER_SEED)
    seen = []

    def ref_detok(toks):
        seen.append(list(toks))
        return spm_ref.decode("uni64", toks).decode("utf-8")

    ora_c, ora_ref = orc.OracleAsr(cfg, B, *tiny_weights), orc.OracleAsr(cfg, B, *tiny_weights)
    be, keep = worker_ref.oracle_backend(dsm, ora_c, cfg, B)
    worker = dsm.Worker(backend=be, tokenizer_file=model_path("uni64"))
    ref = worker_ref.RefWorker(ora_ref, B, cfg.asr_delay_in_tokens, cfg.extra_heads_num, ref_detok)
    run_script(dsm, worker, ref, events, B)
    worker.close()
    assert any(len(t) > 0 for t in seen), "the run must contain a Word with tokens"
    assert any(spm_ref.decode("uni64", t) not in (b"", " ".join(map(str, t)).encode()) for t in seen)

    callback = lambda toks: "cb:" + ",".join(str(t) for t in toks)
    for kw, detok in ((dict(detokenizer=callback, tokenizer_file=model_path("uni64")), callback), (dict(), None)):
        be, keep = worker_ref.oracle_backend(dsm, orc.OracleAsr(cfg, B, *tiny_weights), cfg, B)
        worker = dsm.Worker(backend=be, **kw)
        ref = worker_ref.RefWorker(orc.OracleAsr(cfg, B, *tiny_weights), B, cfg.asr_delay_in_tokens, cfg.extra_heads_num, detok)
        run_script(dsm, worker, ref, events, B)
        worker.close()


def test_worker_step_fails_on_a_token_outside_the_model(dsm, lib, orc, tiny_weights):
    """uni40.model under a 64-entry text vocabulary (a backend that does not state its vocabulary is not checked at set time):
    the first Word with a token >= 40 ends that step with DSM_ERR_STATE and the decoder's message — the `?` of
    srv/batched_asr.rs:667."""
    cfg = dsm.config_tiny()
    B = 4
    be, keep = worker_ref.oracle_backend(dsm, orc.OracleAsr(cfg, B, *tiny_weights), cfg, B)
    worker = dsm.Worker(backend=be, tokenizer_file=model_path("uni40"))
    slots = [worker.open() for _ in range(B)]
    codes = []
    for step_events in worker_ref.script(B, 40, seed=WORKER_SEED):
        for ev in step_events:
            if ev[0] == "audio":
                worker.send(slots[ev[1]], dsm.encode_in_msg("Audio", pcm=ev[2]))
        codes.append(lib.dsm_worker_step(worker.h))
        if codes[-1] < 0:
            break
    assert codes[-1] == DSM_ERR_STATE, codes
    message = lib.dsm_worker_last_error(worker.h).decode()
    assert "out of range" in message and "40 pieces" in message
    worker.close()
