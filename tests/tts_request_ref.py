"""The reference's TTS inference loop (srv/tts.rs:574-621; :852-907 is the same loop over a complete prompt) restated in
Python for B slots over any object with step(prev, allowed, mask) -> (text, audio) or step_pcm(...) -> (text, audio, pcm,
valid): OracleTts on the CPU, a twin TtsEngine on the GPU.  One batched step per loop iteration; a slot that has to wait for
a word (in_rx.recv(), :606) sits iterations out until the script says the word exists.

A generation is a dict: slot, words (token lists, bos already inserted), max_seq_len, extra_steps, and optionally
  at      loop iteration at which the request begins (default 0)
  reset   reset the slot before it begins (a second generation on the slot)
  setup   callable(engine, slot) after the reset (set_ca_src / set_sampling)
  script  [(iteration, n_words, closed)], ascending: from that iteration on the first n_words words exist and the channel is
          closed or not.  Default: every word exists from the start and the channel is closed (a whole prompt)."""
import numpy as np

from dsm_amd import TTS_ALLOW_PAD, TTS_ALLOW_PAD_OR_EPAD

IDLE, RUNNING, WAITING, DONE, DONE_LIMIT = range(5)
UNG = 0xFFFFFFFF


class _Loop:
    def __init__(self, cfg, gen):
        self.cfg, self.gen = cfg, gen
        self.words = [list(w) for w in gen["words"]]
        self.script = gen.get("script") or [(0, len(self.words), True)]
        self.status = RUNNING
        self.step = 0                      # the loop's step_idx == State::step_idx
        self.word = -1                     # Some(vec![]): the empty word that triggers the first bos (:577)
        self.has_word = True
        self.token_idx = self.step_past_last = self.last_epad = self.cpads = 0
        self.last_text = cfg.text_start_token
        self.out = dict(text=[], audio=[], valid=[], pcm=[], kind=[], forced=[], events=[], overwritten=[])

    def avail(self, it):
        n, closed = 0, False
        for at, nw, cl in self.script:
            if at <= it:
                n, closed = nw, cl
        return n, closed

    def take_next(self, it):
        """word_tokens = in_rx.recv(): True when it returned (a word, or None)."""
        n, closed = self.avail(it)
        if self.word + 1 < n:
            self.word += 1
        elif closed:
            self.has_word = False
            self.out["overwritten"].append(self.step - 1)   # overwrite_last_text_token(pad), :609
        else:
            return False
        return True

    def before(self, it, n_steps_limit):
        """The head of a loop iteration: (steps, allowed)."""
        if self.status == WAITING and self.take_next(it):
            self.status = RUNNING
        if self.status != RUNNING:
            return False, TTS_ALLOW_PAD
        cfg = self.cfg
        if self.step >= self.gen["max_seq_len"] or self.step + 1 >= n_steps_limit:
            self.status = DONE_LIMIT
            return False, TTS_ALLOW_PAD
        if not self.has_word:
            self.step_past_last += 1
            if self.step_past_last > self.gen["extra_steps"] + cfg.text_audio_delay_in_tokens:
                self.status = DONE
                return False, TTS_ALLOW_PAD
            self.out["kind"].append("pad")
            return True, TTS_ALLOW_PAD
        w = self.words[self.word] if self.word >= 0 else []
        if self.token_idx < len(w):
            self.out["kind"].append("text")
            return True, int(w[self.token_idx])
        self.out["kind"].append("pad_or_epad")
        return True, TTS_ALLOW_PAD_OR_EPAD

    def after(self, it, tok, audio, pcm, valid):
        cfg, o = self.cfg, self.out
        o["forced"].append(o["kind"][-1] == "pad_or_epad" and self.cpads > cfg.max_consecutive_pads)
        self.cpads = self.cpads + 1 if tok == cfg.text_pad_token else 0
        o["text"].append(int(tok))
        o["audio"].append(np.array(audio, dtype=np.uint32))
        o["valid"].append(int(valid))
        o["pcm"].append(None if pcm is None else np.array(pcm, dtype=np.float32))
        if tok == cfg.text_eop_token:
            if self.has_word:
                o["events"].append((self.word, self.last_epad, self.step))
            self.last_epad = self.step
            if self.has_word:
                self.step += 1     # take_next records step - 1: the step just taken
                if not self.take_next(it):
                    self.status = WAITING
                self.step -= 1
            self.token_idx = 0
        elif tok != cfg.text_pad_token:
            self.token_idx += 1
        self.last_text = int(tok)
        self.step += 1


def run(eng, cfg, B, gens, n_iter, decode=False):
    """Runs the generations for n_iter loop iterations.  Returns (results, stepped): results[i] for gens[i] — the per-step
    lists text / audio / valid / pcm / kind / forced, events [(word, start_step, stop_step)], overwritten (steps whose text-table
    entry became pad), status, step_idx, table (rows of audio_tokens) — and stepped [n_iter][B]."""
    n_limit = cfg.max_steps + cfg.acoustic_delay
    live = {}
    stepped = np.zeros((n_iter, B), dtype=np.uint8)

    def finish(lp):
        lp.out["status"], lp.out["step_idx"] = lp.status, lp.step
        lp.out["table"] = [eng.audio_tokens(lp.gen["slot"], i).copy() for i in range(lp.step)]

    for it in range(n_iter):
        for g in gens:
            if g.get("at", 0) == it:
                b = g["slot"]
                if b in live:
                    finish(live[b])
                if g.get("reset"):
                    eng.reset_batch_idx(b)
                if g.get("setup"):
                    g["setup"](eng, b)
                live[b] = g["_loop"] = _Loop(cfg, g)
        prev = np.zeros(B, dtype=np.uint32)
        allowed = np.full(B, TTS_ALLOW_PAD, dtype=np.int32)
        mask = np.zeros(B, dtype=np.uint8)
        for b, lp in live.items():
            steps, al = lp.before(it, n_limit)
            if steps:
                prev[b], allowed[b], mask[b] = lp.last_text, al, 1
        if not mask.any():
            continue
        stepped[it] = mask
        if decode:
            text, audio, pcm, valid = eng.step_pcm(prev, allowed, mask)
        else:
            (text, audio), pcm, valid = eng.step(prev, allowed, mask), None, np.zeros(B, dtype=np.uint8)
        for b, lp in live.items():
            if mask[b]:
                lp.after(it, text[b], audio[b], None if pcm is None or not valid[b] else pcm[b], valid[b])
    for lp in live.values():
        finish(lp)
    return [g.pop("_loop").out for g in gens], stepped


WEIGHT_SEED = 22  # synthetic weights whose text logits prefer the pad often enough for the forced end-of-pad (found on the oracle)


def tts_setup(dsm, **kw):
    """config_tts_tiny and its synthetic weights at WEIGHT_SEED."""
    import tts_pcm_ref
    from dsm_amd import synth
    cfg_t = dsm.config_tts_tiny(**kw)
    tag = "tts_tiny_s%d" % WEIGHT_SEED + ("_ca" if kw.get("cross_attention") else "")
    return cfg_t, synth.make_synth_tts_weights(cfg_t, tts_pcm_ref.WDIR, seed=WEIGHT_SEED, tag=tag)


def whole_prompts(cfg):
    """The four prompts of the whole-prompt tests (tokens 4.. avoid the special ids; bos = text_bos_token leads the first word):
    slot 0 single-token words with a run of empty words (every one needs an end-of-pad: the PadOrEpad branches, the forced one
    included), slot 1 multi-token words, one with a Text token whose VALUE is the end-of-pad id, slot 2 an empty prompt closed at
    once, slot 3 a prompt cut by max_seq_len."""
    bos, eop = cfg.text_bos_token, cfg.text_eop_token
    return [
        dict(slot=0, words=[[bos, 7]] + [[]] * 28 + [[9], [11]], max_seq_len=64, extra_steps=2),
        dict(slot=1, words=[[bos, 10, 11, 12], [20, eop, 21], [], [14, 15, 16]], max_seq_len=64, extra_steps=1),
        dict(slot=2, words=[], max_seq_len=64, extra_steps=3),
        dict(slot=3, words=[[bos, 30, 31], [32, 33], [34, 35, 36], [37]], max_seq_len=9, extra_steps=0),
    ]


LATE_ITERS = 112  # loop iterations the late schedule needs: seven blocks of 16


def late_prompts(cfg):
    """whole_prompts with words held back: pushes at iterations 16, 32 and 48 (block boundaries at K = 16).  Slot 1 has no word at
    all during block 0 and waits for its third word through the whole of block 2 (iterations 32-47)."""
    gens = whole_prompts(cfg)
    gens[0]["script"] = [(0, 1, False), (16, 12, False), (32, len(gens[0]["words"]), True)]
    gens[1]["script"] = [(0, 0, False), (16, 2, False), (48, 4, True)]
    return gens


def check_branches(cfg, results):
    """Conditions on the INPUTS: the prompts walk every branch of the loop in at least one slot.  Returns the counts."""
    pad, eop = cfg.text_pad_token, cfg.text_eop_token
    n = dict(text=0, poe_pad=0, poe_eop=0, forced=0, pad_tail=0, text_is_eop=0)
    for r in results:
        for kind, forced, tok in zip(r["kind"], r["forced"], r["text"]):
            if kind == "text":
                n["text"] += 1
                n["text_is_eop"] += tok == eop
            elif kind == "pad":
                n["pad_tail"] += 1
            elif forced:
                n["forced"] += 1
                assert tok == eop
            elif tok == pad:
                n["poe_pad"] += 1
            else:
                n["poe_eop"] += 1
    assert all(v > 0 for v in n.values()), n
    assert any(r["status"] == DONE for r in results), [r["status"] for r in results]          # the tail rule
    assert any(r["status"] == DONE_LIMIT for r in results), [r["status"] for r in results]    # max_seq_len
    return n
