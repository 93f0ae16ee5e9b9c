"""Token scores on the GPU (dsm_asr_set_token_scores; csrc/dsm_token_scores.h): lm_token_scores_kernel gives the bits of the host
function — on crafted rows and inside the step, for one and for several stream groups, with greedy and with sampled tokens —,
turning scores on changes no token, no VAD value and no snapshot, word scores follow the word assembly, and the worker's Word
messages carry their mean and minimum.  Floats are compared as uint32."""
import math
import os

import numpy as np
import pytest

from token_scores_cases import NONE, VOCABS, WordAssembly, crafted_rows

pytestmark = pytest.mark.gpu

WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_rows(dsm, eng, text, rows, top_n, V):
    """The step's scores of the listed slots against the host function on that step's logits rows."""
    logits = eng.debug_read("lm.logits", eng.B * V).reshape(eng.B, V)
    lp, ids, lps = eng.token_scores()
    assert ids.shape == (eng.B, top_n) and lps.shape == (eng.B, top_n)
    for b in rows:
        h_lp, h_ids, h_lps = dsm.token_scores_host(logits[b], text[b], top_n)
        assert bits(lp[b]) == bits(h_lp), (b, lp[b], h_lp)
        assert np.array_equal(ids[b], h_ids), (b, ids[b], h_ids)
        assert np.array_equal(bits(lps[b]), bits(h_lps)), (b, lps[b], h_lps)
        assert math.isfinite(lp[b]) and lp[b] <= 0.0
    return lp, ids, lps


def random_codes(cfg, B, steps, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg.audio_vocab_size - 1, (B, cfg.audio_codebooks)).astype(np.uint32) for _ in range(steps)]


def test_kernel_gives_the_bits_of_the_host_function(gpu, dsm, lib, tiny_weights):
    """debug_token_scores runs the step's kernel on the crafted rows of the CPU test: V = 1 .. 8000 leaves lanes of the 256-lane
    sum empty, fills them exactly, or unevenly; ties, -inf entries and V < 8 (padding) are among the rows.  V = 15360 / 15361
    sit on either side of the kernel's LDS-staging threshold."""
    eng = dsm.AsrEngine(dsm.config_tiny(), 2, *tiny_weights)
    for V in VOCABS + (15360, 15361):  # the last two: the longest row the kernel stages in LDS, the shortest it re-reads from L2
        rows, toks = crafted_rows(V)
        lp, ids, lps = eng.debug_token_scores(rows, toks, 8)
        for r in range(rows.shape[0]):
            h_lp, h_ids, h_lps = dsm.token_scores_host(rows[r], toks[r], 8)
            assert bits(lp[r]) == bits(h_lp), (V, r, lp[r], h_lp)
            assert np.array_equal(ids[r], h_ids), (V, r, ids[r], h_ids)
            assert np.array_equal(bits(lps[r]), bits(h_lps)), (V, r, lps[r], h_lps)
    rows, toks = crafted_rows(257)
    for N in (0, 1):  # fewer alternatives than the buffers hold
        lp, ids, lps = eng.debug_token_scores(rows, toks, N)
        for r in range(rows.shape[0]):
            h_lp, h_ids, h_lps = dsm.token_scores_host(rows[r], toks[r], N)
            assert bits(lp[r]) == bits(h_lp) and np.array_equal(ids[r], h_ids) and np.array_equal(bits(lps[r]), bits(h_lps))
    # a row with NaN entries: its scores are unspecified, its ids are entries of the row or padding
    nan_rows = np.stack([np.where(np.arange(300) % 7 == 0, np.nan, rows[0, :1].repeat(300) - np.arange(300)),
                         np.full(300, np.nan)]).astype(np.float32)
    _, ids, _ = eng.debug_token_scores(nan_rows, np.array([1, 0], dtype=np.uint32), 8)
    assert np.all((ids < 300) | (ids == NONE)) and np.all(ids[1] == NONE)
    assert ids[0].tolist() == [j for j in range(300) if j % 7][:8]
    with pytest.raises(dsm.DsmError):
        eng.debug_token_scores(rows, np.full(5, 257, dtype=np.uint32), 8)  # token outside the row: refused on the host
    eng.close()


@pytest.mark.parametrize("model", ["tiny", "medium_bx3"])
def test_scores_in_the_step_with_one_stream_group(gpu, dsm, lib, tiny_weights, model):
    """tiny (V = 64) at B = 3 with slot 1 masked out for 14 steps — the ring of 12 wraps, the step settles into its graph —, and
    a medium model (V = 256, dot_mode 1) at B = 5 for 6 steps: next to a scores-off engine on the same audio the tokens and VAD
    values are the same bits, and each active slot's scores are the host function's on that step's logits row."""
    from dsm_amd import synth
    if model == "tiny":
        cfg, weights, B, steps, mask = dsm.config_tiny(), tiny_weights, 3, 14, np.array([1, 0, 1], dtype=np.uint8)
    else:
        cfg = dsm.config_medium()
        cfg.dot_mode = 1
        weights = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="medium_bf16_hd128_ctx300")
        B, steps, mask = 5, 6, np.ones(5, dtype=np.uint8)
    V = cfg.text_out_vocab_size
    on, off = dsm.AsrEngine(cfg, B, *weights), dsm.AsrEngine(cfg, B, *weights)
    on.set_token_scores(8)
    assert len(on.stream_groups()) == 1
    pcm = synth.synth_pcm(B, steps)
    act = mask.astype(bool)
    for s in range(steps):
        c1, t1, p1 = on.step_pcm(pcm[s], mask)
        c0, t0, p0 = off.step_pcm(pcm[s], mask)
        assert np.array_equal(t1[act], t0[act]) and np.array_equal(c1[act], c0[act]), s
        assert np.array_equal(bits(p1[:, act]), bits(p0[:, act])), s
        _, ids, _ = check_rows(dsm, on, t1, np.flatnonzero(act), 8, V)
        assert np.array_equal(ids[act, 0], t1[act]), s  # temperature 0: the token is the best entry
    m = on.metrics()
    assert m.capture_failures == 0 and off.metrics().capture_failures == 0
    assert m.graph_launches > 0 or steps < 4
    with pytest.raises(dsm.DsmError):
        off.token_scores()  # DSM_ERR_STATE while scores are off
    with pytest.raises(dsm.DsmError):
        off.poll_word_scores()
    on.close()
    off.close()


def test_scores_with_several_stream_groups(gpu, dsm, lib, tiny_weights):
    """B = 130 splits into two stream groups (80 + 50 slots), each with a launch of its own over its rows: the first and the last
    row of every group, three steps."""
    cfg = dsm.config_tiny()
    B, V = 130, cfg.text_out_vocab_size
    on, off = dsm.AsrEngine(cfg, B, *tiny_weights), dsm.AsrEngine(cfg, B, *tiny_weights)
    groups = on.stream_groups()
    assert len(groups) >= 2 and sum(n for _, n in groups) == B
    on.set_token_scores(8)
    rows = sorted({r for b0, n in groups for r in (b0, b0 + n - 1)})
    mask = np.ones(B, dtype=np.uint8)
    for s, codes in enumerate(random_codes(cfg, B, 3, seed=21)):
        t1, p1 = on.step_tokens(codes, mask)
        t0, p0 = off.step_tokens(codes, mask)
        assert np.array_equal(t1, t0) and np.array_equal(bits(p1), bits(p0)), s
        _, ids, _ = check_rows(dsm, on, t1, rows, 8, V)
        assert np.array_equal(ids[rows, 0], t1[rows])
    assert on.metrics().capture_failures == 0
    on.close()
    off.close()


def test_scores_of_sampled_tokens(gpu, dsm, lib, tiny_weights):
    """temperature 0.7: the token is drawn with Gumbel noise, the scores stay those of the raw logits at temperature 1 — the
    sampled token's logprob, and a top list led by the argmax, which the token need not be."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    cfg.temperature = 0.7
    B, V = 3, cfg.text_out_vocab_size
    on, off = dsm.AsrEngine(cfg, B, *tiny_weights), dsm.AsrEngine(cfg, B, *tiny_weights)
    for e in (on, off):
        for b in range(B):
            e.set_seed(b, 700 + b)
    on.set_token_scores(8)
    pcm = synth.synth_pcm(B, 8)
    mask = np.ones(B, dtype=np.uint8)
    differs = 0
    for s in range(8):
        _, t1, _ = on.step_pcm(pcm[s], mask)
        _, t0, _ = off.step_pcm(pcm[s], mask)
        assert np.array_equal(t1, t0), s
        _, ids, _ = check_rows(dsm, on, t1, range(B), 8, V)
        logits = on.debug_read("lm.logits", B * V).reshape(B, V)
        assert np.array_equal(ids[:, 0], np.argmax(logits, axis=1))
        differs += int(np.sum(ids[:, 0] != t1))
    print(f"sampled token != argmax in {differs} of {8 * B} draws")
    assert on.metrics().capture_failures == 0
    on.close()
    off.close()


def test_switching_scores_mid_stream_changes_no_token(gpu, dsm, lib, tiny_weights):
    """4 steps off, 4 with N = 0, 4 with N = 8, 4 off again: every change makes the LM step's graph settle anew (the setting is
    part of its capture key), and the 16 steps give the tokens and VAD values of an engine that never had scores."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    B, V = 3, cfg.text_out_vocab_size
    eng, ref = dsm.AsrEngine(cfg, B, *tiny_weights), dsm.AsrEngine(cfg, B, *tiny_weights)
    pcm = synth.synth_pcm(B, 16)
    mask = np.ones(B, dtype=np.uint8)
    for s in range(16):
        if s % 4 == 0:
            eng.set_token_scores((-1, 0, 8, -1)[s // 4])
            if s in (4, 8):
                with pytest.raises(dsm.DsmError):
                    eng.token_scores()  # no step yet under the new setting
        _, t1, p1 = eng.step_pcm(pcm[s], mask)
        _, t0, p0 = ref.step_pcm(pcm[s], mask)
        assert np.array_equal(t1, t0) and np.array_equal(bits(p1), bits(p0)), s
        top_n = (-1, 0, 8, -1)[s // 4]
        if top_n >= 0:
            check_rows(dsm, eng, t1, range(B), top_n, V)
        else:
            with pytest.raises(dsm.DsmError):
                eng.token_scores()
    for e in (eng, ref):
        assert e.metrics().capture_failures == 0
    with pytest.raises(dsm.DsmError):
        eng.set_token_scores(9)
    with pytest.raises(dsm.DsmError):
        eng.set_token_scores(-2)
    eng.close()
    ref.close()


def test_word_scores_follow_the_word_assembly(gpu, dsm, lib, tiny_weights):
    """Seeded random codes through step_tokens at B = 4 for 60 steps (the CPU oracle on these codes yields 19 words, 15 of them
    of two or more tokens): a word assembly written here from the per-step tokens and token_scores gives, for every Word of
    poll_msgs, exactly the floats poll_word_scores holds at that message's offsets."""
    cfg = dsm.config_tiny()
    B = 4
    eng = dsm.AsrEngine(cfg, B, *tiny_weights)
    eng.set_token_scores(0)
    asm = [WordAssembly(cfg.asr_delay_in_tokens) for _ in range(B)]
    mask = np.ones(B, dtype=np.uint8)
    n_words = n_long = 0
    for s, codes in enumerate(random_codes(cfg, B, 60, seed=1)):
        text, _ = eng.step_tokens(codes, mask)
        lp, _, _ = eng.token_scores()
        want = {b: w for b in range(B) for w in [asm[b].step(text[b], lp[b])] if w is not None}
        words = [m for m in eng.poll_msgs() if m[0] == "Word"]
        scores = eng.poll_word_scores()
        assert sorted(m[1] for m in words) == sorted(want), s
        off = 0
        for _, b, _, toks in words:
            got = scores[off:off + len(toks)]
            off += len(toks)
            assert toks == want[b][0], (s, b)
            assert np.array_equal(bits(got), bits(want[b][1])), (s, b, got, want[b][1])
            assert np.all(np.isfinite(got))
            n_words += 1
            n_long += len(toks) >= 2
        assert off == scores.size
        assert [(b, bits(x).tolist()) for b, x in eng.word_scores()] == [(m[1], bits(want[m[1]][1]).tolist()) for m in words]
    assert n_words >= 5 and n_long >= 1, (n_words, n_long)
    eng.reset_batch_idx(2)  # the pending word's scores go with its tokens
    asm[2].reset()
    eng.close()


def test_snapshots_carry_no_scores_and_do_not_depend_on_them(gpu, dsm, lib, tiny_weights):
    """Slot 1 of A is exported with three tokens of a word pending and imported into slot 0 of C (both with scores on): the
    stream continues there with A's tokens and words; the word that was pending reads NaN for its three pre-import tokens and A's
    own finite scores for the rest, later words are finite throughout.  The blob is byte-equal to the one a scores-off engine
    exports in the same state."""
    cfg = dsm.config_tiny()
    K, CONT = 10, 28
    codes = random_codes(cfg, 3, K + CONT, seed=1)
    other = random_codes(cfg, 1, CONT, seed=2000)
    A, A_off = dsm.AsrEngine(cfg, 3, *tiny_weights), dsm.AsrEngine(cfg, 3, *tiny_weights)
    A.set_token_scores(0)
    asm = WordAssembly(cfg.asr_delay_in_tokens)
    ones3, ones2 = np.ones(3, dtype=np.uint8), np.ones(2, dtype=np.uint8)
    for s in range(K):
        text, _ = A.step_tokens(codes[s], ones3)
        t_off, _ = A_off.step_tokens(codes[s], ones3)
        assert np.array_equal(text, t_off)
        asm.step(text[1], A.token_scores()[0][1])
    n_pending = len(asm.tokens)
    assert n_pending >= 2, "precondition: slot 1 holds a pending word at the export"
    blob = A.export_slots([1])
    assert blob == A_off.export_slots([1])
    A_off.close()
    C = dsm.AsrEngine(cfg, 2, *tiny_weights)
    C.set_token_scores(0)
    C.import_slots([0], blob)
    words = straddling = 0
    for s in range(K, K + CONT):
        ta, _ = A.step_tokens(codes[s], ones3)
        wa = [(m[3], x) for m, (_, x) in zip([m for m in A.poll_msgs() if m[0] == "Word"], A.word_scores()) if m[1] == 1]
        tc, _ = C.step_tokens(np.stack([codes[s][1], other[s - K][0]]), ones2)
        wc = [(m[3], x) for m, (_, x) in zip([m for m in C.poll_msgs() if m[0] == "Word"], C.word_scores()) if m[1] == 0]
        assert tc[0] == ta[1], s
        assert [w[0] for w in wc] == [w[0] for w in wa], s
        for (toks, got), (_, src) in zip(wc, wa):
            assert np.all(np.isfinite(src))
            first = words == 0
            k = n_pending if first else 0
            assert np.all(np.isnan(got[:k])) and np.array_equal(bits(got[k:]), bits(src[k:])), (s, got, src)
            straddling += first and len(toks) > n_pending
            words += 1
    assert words >= 2 and straddling == 1, (words, straddling)
    A.close()
    C.close()


def test_worker_words_carry_mean_and_minimum_logprob(gpu, dsm, lib, tiny_weights):
    """The same 40 noise frames on two slots through three workers on tiny engines (the CPU oracle yields four Words on them):
    with set_word_scores(1) every Word decoded with msgpack carries logprob and min_logprob, the f64 mean and minimum of the engine's
    scores for that word; switched off again before the first frame — engine scores still on — the wire bytes are those of a
    worker that never heard of the call."""
    import ctypes as C
    import msgpack
    cfg = dsm.config_tiny()
    B, frames = 2, 40
    rng = np.random.default_rng(12)
    audio = [(0.1 * rng.standard_normal((B, 1920))).astype(np.float32) for _ in range(frames)]

    def run(mode):
        eng = dsm.AsrEngine(cfg, B, *tiny_weights)
        w = dsm.Worker(eng)
        if mode != "never":
            w.set_word_scores(True)
        if mode == "off":
            w.set_word_scores(False)
        slots = [w.open() for _ in range(B)]
        raw, want = {s: [] for s in slots}, {s: [] for s in slots}
        buf, n = np.zeros(1 << 16, dtype=np.uint8), C.c_size_t(0)
        for f in range(frames):
            for s in slots:
                w.send(s, dsm.encode_in_msg("Audio", pcm=audio[f][s]))
            assert w.step()
            if mode == "on":
                words = [m for m in eng.poll_msgs() if m[0] == "Word"]
                for m, (b, lps) in zip(words, eng.word_scores()):
                    assert m[1] == b and np.all(np.isfinite(lps))
                    want[b].append((sum(float(x) for x in lps) / len(lps), min(float(x) for x in lps)))
            for s in slots:
                while lib.dsm_worker_recv(w.h, s, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == 1:
                    raw[s].append(buf[:n.value].tobytes())
        w.close()
        eng.close()
        return raw, want

    raw_on, want = run("on")
    n_words = 0
    for s, msgs in raw_on.items():
        got = [m for m in map(msgpack.unpackb, msgs) if m["type"] == "Word"]
        assert len(got) == len(want[s])
        for m, (mean, low) in zip(got, want[s]):
            assert list(m) == ["type", "text", "start_time", "logprob", "min_logprob"]
            assert m["logprob"] == mean and m["min_logprob"] == low and low <= mean <= 0.0
            n_words += 1
        assert all(dsm.decode_out_msg(r)["type"] == msgpack.unpackb(r)["type"] for r in msgs)  # the project's decoder skips the new keys
    assert n_words >= 2
    raw_off, _ = run("off")
    raw_never, _ = run("never")
    assert raw_off == raw_never
    words_never = [m for s in raw_never for m in map(msgpack.unpackb, raw_never[s]) if m["type"] == "Word"]
    assert len(words_never) == n_words and all(list(m) == ["type", "text", "start_time"] for m in words_never)
    # apart from the two keys the messages are the same
    strip = lambda m: {k: v for k, v in m.items() if k not in ("logprob", "min_logprob")}
    assert {s: [strip(msgpack.unpackb(r)) for r in raw_on[s]] for s in raw_on} == \
           {s: [msgpack.unpackb(r) for r in raw_never[s]] for s in raw_never}
