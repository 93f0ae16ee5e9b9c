"""The native tokenizer at the two ends of the served loops, on the engine.  STT: Word.text of a worker with
tokenizer_file = uni64.model against RefWorker with tests/spm_ref.py (the decode restatement test_spm_cpu.py pins to Python
sentencepiece), single-call and two-thread.  TTS: a request fed text (dsm_tts_request_push_text) against its twin slot fed the
recorded ids (dsm_tts_request_push_words) — every token, event and status the same — and dsm_tts_word_text of every event."""
import threading
import time

import numpy as np
import pytest

import spm_ref
import tts_request_ref as Q
import worker_ref
from test_spm_cpu import model_path
from test_worker_cpu import run_script

pytestmark = pytest.mark.gpu
DSM_ERR_INVALID, DSM_ERR_STATE = -1, -4


def test_worker_word_text_on_the_engine(gpu, dsm, lib, orc, tiny_weights):
    cfg = dsm.config_tiny()
    B = 4
    seen = []

    def ref_detok(toks):
        seen.append(list(toks))
        return spm_ref.decode("uni64", toks).decode("utf-8")

    eng = dsm.AsrEngine(cfg, B, *tiny_weights)
    worker = dsm.Worker(engine=eng, tokenizer_file=model_path("uni64"))
    ref = worker_ref.RefWorker(orc.OracleAsr(cfg, B, *tiny_weights), B, cfg.asr_delay_in_tokens, cfg.extra_heads_num, ref_detok)
    run_script(dsm, worker, ref, worker_ref.script(B, 60, seed=8), B)
    assert any(len(t) > 0 for t in seen), "the run must contain a Word with tokens"
    worker.close()
    eng.close()


def test_engine_worker_refuses_a_tokenizer_beyond_its_vocabulary(gpu, dsm, lib, tiny_weights):
    """config_tiny's text_out_vocab_size is 64: the 512-piece model is refused at set time, the 64-piece one is taken."""
    eng = dsm.AsrEngine(dsm.config_tiny(), 2, *tiny_weights)
    worker = dsm.Worker(engine=eng)
    with pytest.raises(dsm.DsmError, match="512 pieces") as ei:
        worker.set_tokenizer_file(model_path("uni512_nfkc_bf"))
    assert ei.value.code == DSM_ERR_INVALID
    worker.set_tokenizer_file(model_path("uni64"))
    worker.close()
    eng.close()


def test_two_thread_worker_delivers_the_same_word_text(gpu, dsm, lib, tiny_weights):
    """dsm_worker_step_encode / dsm_worker_step_model on two threads with a tokenizer: the bytes of dsm_worker_step."""
    cfg = dsm.config_tiny()
    B, frames = 4, 40
    rng = np.random.default_rng(9)
    audio = [[(0.1 * rng.standard_normal(1920 + int(rng.integers(0, 3)) * 64)).astype(np.float32) for _ in range(frames)] for _ in range(B)]

    def feed(w, slots, f):
        for slot in slots:
            w.send(slot, dsm.encode_in_msg("Audio", pcm=audio[slot][f]))

    ea = dsm.AsrEngine(cfg, B, *tiny_weights)
    wa = dsm.Worker(ea, tokenizer_file=model_path("uni64"))
    sa = [wa.open() for _ in range(B)]
    for f in range(frames):
        feed(wa, sa, f)
        assert wa.step()
    while wa.step():  # queued remainders
        pass
    want = {s: wa.recv(s) for s in sa}
    wa.close(); ea.close()
    words = [m["text"] for s in sa for m in want[s] if m["type"] == "Word"]
    assert any(words), "the run must contain a Word with tokens"
    assert not any(w and all(p.isdigit() for p in w.split(" ")) for w in words), "decimal ids: the tokenizer was not used"

    eb = dsm.AsrEngine(cfg, B, *tiny_weights)
    wb = dsm.Worker(eb, tokenizer_file=model_path("uni64"))
    sb = [wb.open() for _ in range(B)]
    assert sb == sa
    count = {"encoded": 0, "stepped": 0}
    errors, done = [], threading.Event()

    def encoder_loop():
        try:
            for f in range(frames):
                feed(wb, sb, f)
                while not wb.step_encode():  # queue full: the model side is three frames behind
                    time.sleep(0)
                count["encoded"] += 1
            while True:  # drain the remainders: idle is told from a full queue by letting the model side catch up first
                while count["stepped"] < count["encoded"] and not errors:
                    time.sleep(0)
                if errors or not wb.step_encode():
                    break
                count["encoded"] += 1
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
        done.set()

    def model_loop():
        try:
            while True:
                if wb.step_model():
                    count["stepped"] += 1
                elif done.is_set():
                    break
                else:
                    time.sleep(0)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)

    te, tm = threading.Thread(target=encoder_loop), threading.Thread(target=model_loop)
    te.start(); tm.start(); te.join(120); tm.join(120)
    assert not errors, errors
    got = {s: wb.recv(s) for s in sb}
    for s in sa:
        assert got[s] == want[s], f"slot {s}: the two-thread worker delivered different messages"
    wb.close(); eb.close()


# ---- TTS ----
# two client messages; runs of spaces make empty words, which are skipped.  19 tokens with the bos and 5 word ends of at most
# max_consecutive_pads + 1 steps each, then the tail: the request ends well inside config_tts_tiny's 64 steps
MESSAGES = ["the  engine ", "frames now"]
WORDS = [["the", "engine"], ["frames", "now"]]


def recorded_ids(word):
    for text_hex, ids in spm_ref.vectors()["models"]["uni40"]["encode"]:
        if bytes.fromhex(text_hex) == word.encode():
            return ids
    raise KeyError(word)


def test_tts_text_calls_without_a_tokenizer_and_attach_refusals(gpu, dsm, lib):
    cfg_t, tts_path = Q.tts_setup(dsm)
    eng = dsm.TtsEngine(cfg_t, 2, tts_path)
    eng.request_begin(0, 64, 1)
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*attach_tokenizer"):
        eng.push_text(0, "the engine")
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*attach_tokenizer"):
        eng.word_text(0, -1)
    with pytest.raises(dsm.DsmError, match=r"dsm error -1: .*64 pieces.*40"):  # config_tts_tiny: text_out_vocab_size = 40
        eng.attach_tokenizer(model_path("uni64"))
    with pytest.raises(dsm.DsmError, match=r"dsm error -1: .*BPE"):
        eng.attach_tokenizer(model_path("bpe64"))
    eng.attach_tokenizer(model_path("uni40"))
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*already"):
        eng.attach_tokenizer(model_path("uni40"))
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*no request"):
        eng.push_text(1, "the engine")
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*no request"):
        eng.word_text(1, -1)
    assert eng.push_text(0, "   ") == 0  # nothing but spaces: no word
    eng.request_close(0)
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*closed"):
        eng.push_text(0, "the engine")
    eng.close()


def test_tts_push_text_equals_push_words(gpu, dsm, lib):
    """Slot 0 is fed text in two messages, the second after the first block; slot 1 the recorded ids of the same words with the
    bos in front of the first.  Argmax, run(K = 4) until DONE: the two slots must agree on everything.  Two overflowing
    push_text calls on slot 0 — one before its first word, one between the messages — must change nothing, the first-word flag
    included: the agreement with slot 1 shows it."""
    cfg_t, tts_path = Q.tts_setup(dsm)
    K, B = 4, 2
    eng = dsm.TtsEngine(cfg_t, B, tts_path)
    eng.attach_tokenizer(model_path("uni40"))
    bos = cfg_t.text_bos_token
    ids = [[recorded_ids(w) for w in msg] for msg in WORDS]
    pushed = [[bos] + ids[0][0]] + ids[0][1:] + ids[1]  # per word, as slot 1 pushes them
    too_long = " ".join(["a"] * (cfg_t.max_steps + cfg_t.acoustic_delay + 1))  # one word more than the queue holds

    for b in range(B):
        eng.request_begin(b, 64, 1)
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*queue"):
        eng.push_text(0, too_long)
    assert eng.push_text(0, MESSAGES[0]) == len(WORDS[0])
    eng.push_words(1, pushed[:len(WORDS[0])])

    blocks, events = [], [[], []]
    for it in range(24):
        eng.run(K)
        blk = eng.collect()
        blocks.append(blk)
        for b, w, a, z in blk.events:
            events[b].append((w, a, z))
        if it == 0:
            status = eng.request_status(0)
            with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*queue"):
                eng.push_text(0, too_long)
            assert eng.request_status(0) == status
            assert eng.push_text(0, MESSAGES[1]) == len(WORDS[1])  # no second bos: "first word" is per request
            eng.push_words(1, pushed[len(WORDS[0]):])
            for b in range(B):
                eng.request_close(b)
        if all(eng.request_status(b) in (Q.DONE, Q.DONE_LIMIT) for b in range(B)):
            break
    assert [eng.request_status(b) for b in range(B)] == [Q.DONE, Q.DONE]
    for i, blk in enumerate(blocks):
        assert np.array_equal(blk.stepped[:, 0], blk.stepped[:, 1]), f"block {i}: stepped differs"
        assert np.array_equal(blk.text_token[:, 0], blk.text_token[:, 1]), f"block {i}: text tokens differ"
        assert np.array_equal(blk.audio[:, 0], blk.audio[:, 1]), f"block {i}: audio tokens differ"
        assert blk.status[0] == blk.status[1], f"block {i}: status differs"
    assert events[0] == events[1]
    assert [w for w, _, _ in events[0]] == list(range(-1, len(pushed))), "one event per word, the initial empty word first"
    for b in range(B):
        for w, _, _ in events[b]:
            assert eng.word_text(b, w) == (b"" if w < 0 else spm_ref.decode("uni40", pushed[w]))
        assert eng.word_text(b, -1) == b""
    assert eng.word_text(0, 0) == b"the" and eng.word_text(0, len(pushed) - 1) == b"now"  # the bos decodes to nothing
    with pytest.raises(dsm.DsmError, match=r"dsm error -1: .*no word"):
        eng.word_text(0, len(pushed))
    eng.reset_batch_idx(0)  # the word tokens are kept until here
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*no request"):
        eng.word_text(0, 0)
    eng.close()
