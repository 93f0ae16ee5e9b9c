"""Voices (dsm_tts_voice_create / dsm_tts_set_voice): a cross-attention source projected once into device memory that slots attach
to by reference.  Three engines run the same schedule (tests/tts_schedule.py): one whose slots take VOICES, a twin whose slots
take the same rows through set_ca_src, and the oracle with set_ca_src (it never learns that voices exist).  Text tokens,
depformer tokens and lm.hidden of every batch row that both sides run are compared bit for bit at every step, the audio_tokens
tables at the end."""
import os

import numpy as np
import pytest

import tts_request_ref as Q
from tts_schedule import schedule

pytestmark = pytest.mark.gpu
WDIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")


def _cfg(dsm, variant="", **kw):
    """config_tts_tiny(cross_attention=True) in the three shapes whose cross-attention launch runs another attention instance."""
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny(cross_attention=True, **kw)
    tag = "tts_tiny_ca"
    if variant == "hd64":  # head_dim 64, sources of at most 32 rows: attn_small_kernel
        cfg.lm.num_heads, cfg.depformer.num_heads = 2, 1
        tag += "_hd64"
    elif variant == "hd128":  # head_dim 128 and more than 32 rows: attn_kernel<., 128, 1>, the instance the shipped model runs
        cfg.lm.d_model, cfg.lm.num_heads, cfg.ca_max_len = 256, 2, 40
        tag += "_hd128"
    return cfg, synth.make_synth_tts_weights(cfg, WDIR, tag=tag)


class Trio:
    """eng (voices), twin (private rows), ora (private rows).  A source is (rows, seed) or None; equal sources share one voice."""

    def __init__(self, dsm, orc, cfg, path, B, oracle=True):
        self.cfg, self.B, self.rps = cfg, B, 2 if cfg.cfg_rows else 1
        self.eng, self.twin = dsm.TtsEngine(cfg, B, path), dsm.TtsEngine(cfg, B, path)
        self.ora = orc.OracleTts(cfg, B, path) if oracle else None
        self.voices, self.guided, self.step_no = {}, set(), 0

    def all(self):
        return [x for x in (self.eng, self.twin, self.ora) if x is not None]

    def rows(self, src):
        from dsm_amd import synth
        return None if src is None else synth.synth_ca_src(self.cfg, *src)

    def voice(self, src):
        if src is None:
            return 0
        if src not in self.voices:
            self.voices[src] = self.eng.voice_create(self.rows(src))
        return self.voices[src]

    def source(self, slot, cond, uncond=None, alpha=0.0, private=False):
        """The slot's source on all three; the voice engine attaches voices unless private."""
        for x in self.all():
            if x is self.eng and not private:
                x.set_voice(slot, self.voice(cond), self.voice(uncond), alpha)
            else:
                x.set_ca_src(slot, self.rows(cond), self.rows(uncond), alpha)
        (self.guided.add if uncond is not None else self.guided.discard)(slot)

    def reset(self, slot):
        for x in self.all():
            x.reset_batch_idx(slot)
        self.guided.discard(slot)

    def sampling(self, slot, k, temp, seed):
        for x in self.all():
            x.set_sampling(slot, k, temp, seed)

    def hidden(self, x, mask):
        """lm.hidden of the batch rows that ran: row 0 of every active slot, row 1 of the guided ones among them."""
        R, d = self.B * self.rps, self.cfg.lm.d_model
        h = x.debug_read("lm.hidden", R * d).reshape(self.B, self.rps, d).view(np.uint32)
        return [h[b, j] for b in range(self.B) if mask[b] for j in range(self.rps) if j == 0 or b in self.guided]

    def run(self, sched, events=None):
        for prev, allowed, mask in sched:
            s = self.step_no
            if events and s in events:
                events[s](self)
            act = mask.astype(bool)
            outs = [(x.step(prev, allowed, mask), self.hidden(x, mask)) for x in self.all()]
            (te, ae), he = outs[0]
            for ((t, a), h), who in zip(outs[1:], ("twin", "oracle")):
                assert np.array_equal(te[act], t[act]), f"text tokens differ from the {who}'s at step {s}: {te[act]} vs {t[act]}"
                assert np.array_equal(ae[act], a[act]), f"depformer tokens differ from the {who}'s at step {s}"
                assert len(he) == len(h) and all(np.array_equal(x, y) for x, y in zip(he, h)), f"lm.hidden bits differ from the {who}'s at step {s}"
            self.step_no += 1

    def finish(self):
        for x in self.all()[1:]:
            for b in range(self.B):
                assert self.eng.step_idx(b) == x.step_idx(b)
                for i in range(self.eng.step_idx(b)):
                    assert np.array_equal(self.eng.audio_tokens(b, i), x.audio_tokens(b, i)), f"audio_tokens[{b}][{i}] differ"
        for x in (self.eng, self.twin):
            m = x.metrics()
            assert m.capture_failures == 0, m.capture_error
        for x in self.all():
            x.close()


@pytest.mark.parametrize("kv_bf16", [1, 0])
@pytest.mark.parametrize("variant", ["", "hd64", "hd128"])
def test_voices_equal_private_rows(gpu, dsm, lib, orc, variant, kv_bf16):
    """The swap of test_tts_ca_gpu.py with voices: the longest source allowed, a single row, none, a ragged one; at step 11 slot 1
    is reset and takes a different, longer voice and slot 3 loses its source."""
    cfg, path = _cfg(dsm, variant)
    cfg.kv_bf16 = kv_bf16
    B = 4
    t = Trio(dsm, orc, cfg, path, B)
    for b, n in enumerate([cfg.ca_max_len, 1, 0, 13]):
        if n:
            t.source(b, (n, 50 + b))

    def swap(t):
        t.reset(1)
        t.source(1, (17, 77))
        t.source(3, None)

    t.run(schedule(cfg, B, 26), events={11: swap})
    assert t.eng.voice_info(t.voices[(17, 77)]) == (17, 1, 2 * cfg.lm.num_layers * cfg.lm.d_model * cfg.ca_max_len * (2 if kv_bf16 else 4))
    assert t.eng.voice_info(t.voices[(1, 51)])[1] == 0 and t.eng.voice_info(t.voices[(13, 53)])[1] == 0
    t.finish()


V, U = (20, 1), (9, 99)


def _shared(t):
    """Slots 0, 1, 2 on one voice and one unconditional voice (alpha 2.5, alpha 1.0, unguided), slot 3 on private rows in the same
    engine; slots 1 and 2 sample with different seeds: shared rows must not make slots depend on each other."""
    t.source(0, V, U, 2.5)
    t.source(1, V, U, 1.0)
    t.source(2, V)
    t.source(3, (8, 2), private=True)
    t.sampling(1, 5, 0.8, 42)
    t.sampling(2, 6, 0.9, 1234)
    assert t.eng.voice_info(t.voices[V])[:2] == (20, 3) and t.eng.voice_info(t.voices[U])[:2] == (9, 2)
    assert len(t.voices) == 2


def test_slots_share_a_voice_with_guidance(gpu, dsm, lib, orc):
    cfg, path = _cfg(dsm, cfg_rows=True)
    t = Trio(dsm, orc, cfg, path, 4)
    _shared(t)
    t.run(schedule(cfg, 4, 20))
    t.finish()


def test_a_voice_shared_across_two_stream_groups(gpu, dsm, lib, orc, monkeypatch):
    """DSM_TTS_GROUPS = 2: slots 0-1 and 2-3 step on different streams, each through its r0-offset view of the pointer tables."""
    monkeypatch.setenv("DSM_TTS_GROUPS", "2")
    cfg, path = _cfg(dsm, cfg_rows=True)
    t = Trio(dsm, orc, cfg, path, 4)
    _shared(t)
    t.run(schedule(cfg, 4, 20))
    t.finish()


def test_the_request_path_reads_voices(gpu, dsm, lib):
    """request_begin / push_words / request_close, run(4) + collect until every slot is DONE: two slots share a voice (one guided),
    one has private rows, against the twin driven the same way.  Every block's records are equal."""
    from dsm_amd import synth
    cfg, path = Q.tts_setup(dsm, cross_attention=True, cfg_rows=True)
    rows, empty, other = synth.synth_ca_src(cfg, 20, 1), synth.synth_ca_src(cfg, 9, 99), synth.synth_ca_src(cfg, 8, 2)

    def drive(voices):
        eng = dsm.TtsEngine(cfg, 4, path)
        if voices:
            v, u = eng.voice_create(rows), eng.voice_create(empty)
            eng.set_voice(0, v, u, 2.5)
            eng.set_voice(1, v)
        else:
            eng.set_ca_src(0, rows, empty, 2.5)
            eng.set_ca_src(1, rows)
        eng.set_ca_src(2, other)
        eng.set_sampling(1, 5, 0.8, 1234)
        for g in Q.whole_prompts(cfg):
            eng.request_begin(g["slot"], g["max_seq_len"], g["extra_steps"])
            if g["words"]:
                eng.push_words(g["slot"], g["words"])
            eng.request_close(g["slot"])
        blocks = []
        while any(eng.request_status(b) not in (Q.DONE, dsm.TTS_REQ_DONE_LIMIT) for b in range(4)):
            assert len(blocks) < 40, "the requests do not end"
            eng.run(4)
            blk = eng.collect()
            st = blk.stepped.astype(bool)
            blocks.append((blk.n_steps, blk.stepped.tolist(), blk.text_token[st].tolist(), blk.audio[st].tolist(), blk.events, blk.status.tolist()))
        assert eng.metrics().capture_failures == 0
        tables = [[eng.audio_tokens(b, i).tolist() for i in range(eng.step_idx(b))] for b in range(4)]
        eng.close()
        return blocks, tables

    got, want = drive(True), drive(False)
    assert len(got[0]) == len(want[0]) >= 4
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, f"block {i} differs"
    assert got[1] == want[1]


def test_a_voice_attached_after_the_step_graphs_exist(gpu, dsm, lib, orc):
    """Six steps on private rows (the graphs are captured and replayed), then one slot is reset and put on a voice created NOW:
    a launch argument frozen at capture would still read the private block."""
    cfg, path = _cfg(dsm)
    B = 4
    t = Trio(dsm, orc, cfg, path, B)
    for b in range(B):
        t.source(b, (5 + 4 * b, 30 + b), private=True)
    sched = schedule(cfg, B, 16)
    t.run(sched[:6])
    assert not t.voices
    t.reset(2)
    t.source(2, (19, 61))
    assert t.eng.voice_info(t.voices[(19, 61)])[:2] == (19, 1)
    t.run(sched[6:])
    t.finish()


def test_lifetime_and_errors(gpu, dsm, lib, orc):
    """Every refusal is a checked return code; nothing is freed while a row reads it."""
    from dsm_amd import synth
    cfg, path = _cfg(dsm)
    B = 2
    t = Trio(dsm, orc, cfg, path, B, oracle=False)
    eng = t.eng
    t.source(0, (7, 3))
    t.source(1, (7, 3))
    v = t.voices[(7, 3)]
    with pytest.raises(dsm.DsmError, match="in use by 2 rows"):
        eng.voice_destroy(v)
    sched = schedule(cfg, B, 6)
    t.run(sched[:2])  # the voice still works
    with pytest.raises(dsm.DsmError, match="fresh slot"):
        eng.set_voice(0, v)
    with pytest.raises(dsm.DsmError, match="cfg_rows"):
        eng.set_voice(1, v, v, 2.0)  # an unconditional voice on an engine without cfg_rows (refused before the step index is looked at)
    for bad in (np.zeros((0, cfg.lm.d_model), np.float32), synth.synth_ca_src(cfg, cfg.ca_max_len + 1, 5)):
        with pytest.raises(dsm.DsmError, match="ca_max_len"):
            eng.voice_create(bad)
    # set_ca_src on a slot that holds a voice drops the reference, and the slot computes from the private rows
    t.reset(1)
    eng.set_voice(1, v)
    assert eng.voice_info(v)[1] == 2
    t.source(1, (11, 8), private=True)
    assert eng.voice_info(v)[1] == 1
    t.run(sched[2:4])
    t.reset(0)
    assert eng.voice_info(v) == (7, 0, 2 * cfg.lm.num_layers * cfg.lm.d_model * cfg.ca_max_len * 2)
    eng.voice_destroy(v)
    for call in (lambda: eng.set_voice(0, v), lambda: eng.voice_info(v), lambda: eng.voice_destroy(v), lambda: eng.set_voice(0, 12345)):
        with pytest.raises(dsm.DsmError, match="no voice"):
            call()
    # two voices from the same rows: different handles (never reused), the same tokens
    v1, v2 = eng.voice_create(t.rows((7, 3))), eng.voice_create(t.rows((7, 3)))
    assert len({v, v1, v2}) == 3
    t.voices[(7, 3)] = v2
    t.source(0, (7, 3))  # the twin takes the rows again; slot 1 keeps its private ones
    assert eng.voice_info(v2)[1] == 1 and eng.voice_info(v1)[1] == 0
    t.run(sched[4:])
    tok_v2 = [eng.audio_tokens(0, i).copy() for i in range(eng.step_idx(0))]
    eng.reset_batch_idx(0)
    t.twin.reset_batch_idx(0)
    eng.set_voice(0, v1)
    t.twin.set_ca_src(0, t.rows((7, 3)))
    t.step_no = 4
    t.run(sched[4:])
    assert all(np.array_equal(a, eng.audio_tokens(0, i)) for i, a in enumerate(tok_v2)) and len(tok_v2) == eng.step_idx(0) > 0
    t.finish()
    plain_cfg = dsm.config_tts_tiny()
    plain = dsm.TtsEngine(plain_cfg, B, synth.make_synth_tts_weights(plain_cfg, WDIR, tag="tts_tiny"))
    with pytest.raises(dsm.DsmError, match="cross_attention"):
        plain.voice_create(synth.synth_ca_src(cfg, 4, 1))
    plain.close()
