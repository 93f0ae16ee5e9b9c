"""Text bias on the GPU (dsm_asr_set_text_bias; csrc/dsm_text_bias.h): lm_pick_biased_kernel gives the token and the node of the
host function — on crafted rows and inside the step, with greedy and with sampled tokens, for one and for several stream groups
—, the switch with nothing attached changes nothing, token scores stay those of the raw row, and sets, attachments, resets,
snapshots and the worker behave as include/dsm.h says.  Floats are compared as uint32."""
import ctypes as C
import os

import numpy as np
import pytest

import text_bias_ref as R
from text_bias_ref import DEAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
SPM_MODEL = os.path.join(ROOT, "tests", "golden", "spm", "uni64.model")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_codes(cfg, B, steps, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg.audio_vocab_size - 1, (B, cfg.audio_codebooks)).astype(np.uint32) for _ in range(steps)]


def seed_key(orc, seed):
    key = (C.c_uint32 * 8)()
    orc.lib().orc_seed_from_u64(seed, key)
    return np.array(list(key), dtype=np.uint32)


def resized_tiny(dsm, V):
    """config_tiny with another text_out_vocab_size, and synthetic weights of that shape."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    cfg.text_out_vocab_size = V
    return cfg, synth.make_synth_weights(cfg, WEIGHTS_DIR, tag=f"tiny_vout{V}")


class Follower:
    """The host function beside an engine: per attached slot its set's table and the node the next pick runs at."""

    def __init__(self, dsm, eng, V, temperature=0.0):
        self.dsm, self.eng, self.V, self.temperature = dsm, eng, V, temperature
        self.table, self.node, self.key, self.pos = {}, {}, {}, {}
        self.returns = self.live = self.dead = self.differs = 0
        self.per_slot = {}  # slot -> [returns, live, dead, differs]

    def attach(self, slot, handle, table, node=0):
        self.eng.set_bias(slot, handle)
        self.table[slot], self.node[slot] = table, node
        self.per_slot.setdefault(slot, [0, 0, 0, 0])
        assert self.eng.bias_state(slot) == (handle, node)

    def check(self, step, text, active):
        logits = self.eng.debug_read("lm.logits", self.eng.B * self.V).reshape(self.eng.B, self.V)
        for b in sorted(self.table):
            handle, node = self.eng.bias_state(b)
            if b not in active:
                assert node == self.node[b], (step, b, "an inactive slot's node moved")
                continue
            prev = self.node[b]
            tok, nxt = self.dsm.text_bias_pick_host(self.table[b], prev, logits[b], self.temperature, self.key.get(b), self.pos.get(b, 0))
            assert (int(text[b]), node) == (tok, nxt), (step, b, prev, int(text[b]), node, tok, nxt)
            if self.temperature > 0:
                self.pos[b] += 16 * ((self.V + 15) // 16)
            what = [step > 0 and prev != 0 and nxt == 0, prev not in (0, DEAD), prev == DEAD, tok != R.first_max(logits[b])]
            self.per_slot[b] = [n + bool(w) for n, w in zip(self.per_slot[b], what)]
            self.returns, self.live, self.dead, self.differs = (sum(c[i] for c in self.per_slot.values()) for i in range(4))
            self.node[b] = nxt


def wide_set(V, rng):
    """More than 256 token biases, a root with more than 256 edges and an inner node with more than 256: the strided walks."""
    toks = [(int(t), float(v)) for t, v in zip(rng.choice(V, 300, replace=False), rng.standard_normal(300) * 3)]
    toks[0] = (toks[0][0], -np.inf)
    pieces = [int(p) for p in rng.choice(np.arange(4, V), 600, replace=False)]
    kws = [([p], float(rng.uniform(0.5, 6))) for p in pieces[:300]]
    kws += [([pieces[7], p], float(rng.uniform(0.5, 6))) for p in pieces[300:600]]
    kws += [([pieces[7], pieces[300], pieces[1]], 9.0)]
    return toks, kws, pieces[7]


def test_kernel_gives_the_token_and_node_of_the_host_function(gpu, dsm, lib, orc):
    """debug_text_pick runs the step's kernel on the crafted rows of the CPU test at V = 5 .. 15360 (the longest row the kernel
    stages), at temperature 0 and at 0.7 / 1.0 with given keys and positions; from V = 4000 on also on a set whose lists are
    longer than the workgroup.  The engine's vocabulary is 15360, so one engine holds every set."""
    cfg, weights = resized_tiny(dsm, 15360)
    eng = dsm.AsrEngine(cfg, 2, *weights)
    rng = np.random.default_rng(11)
    crafted = eng.bias_create(*R.crafted_set())
    assert eng.bias_info(crafted) == dict(nodes=6, edges=5, tokens=3, refs=0, device_bytes=4 * (8 + 6 + 7 + 15))
    for V in (5, 64, 255, 256, 257, 4000, 8000, 15360):
        cases = [(crafted, dsm.text_bias_compile(*R.crafted_set(), V), R.crafted_rows(V))]
        if V >= 4000:
            toks, kws, branch = wide_set(V, rng)
            h = eng.bias_create(toks, kws)
            table = dsm.text_bias_compile(toks, kws, 15360)
            info = eng.bias_info(h)
            assert info["tokens"] == 300 and info["nodes"] == 602 and table[4] == 602
            _, nodes = R.parse(table)
            inner = nodes[0][branch][1]
            assert len(nodes[0]) == 300 and len(nodes[inner]) == 300
            rows = []
            for node in (0, inner, DEAD, 0, inner, 1, 601):
                r = (rng.standard_normal(V) * 2).astype(np.float32)
                rows.append((r, node))
            r = np.full(V, -2.0, dtype=np.float32)  # flat: the largest boost decides, ties go to the lower id
            rows += [(r, 0), (r, inner), (r, DEAD)]
            cases.append((h, table, rows))
        cases.append((0, None, R.crafted_rows(V)[:6]))  # no set
        for handle, table, rows in cases:
            logits = np.stack([r for r, _ in rows])
            nodes_in = np.array([n for _, n in rows], dtype=np.uint32)
            for temperature in (0.0, 0.7, 1.0):
                keys = np.stack([seed_key(orc, 900 + i) for i in range(len(rows))])
                pos = np.array([16 * (i * 37 % 11) * ((V + 15) // 16) for i in range(len(rows))], dtype=np.uint64)
                pos[-1] = 2 ** 33 + 16  # beyond 32 bits
                toks_out, nodes_out = eng.debug_text_pick(handle, logits, nodes_in, temperature, keys, pos)
                for i, (row, node) in enumerate(rows):
                    want = dsm.text_bias_pick_host(table, node, row, temperature, keys[i], int(pos[i]))
                    assert (int(toks_out[i]), int(nodes_out[i])) == want, (V, handle, temperature, i, node)
                    if temperature == 0.0 and table is not None:
                        assert want == R.pick_ref(table, node, row)
            if handle not in (0, crafted):
                eng.bias_destroy(handle)
    with pytest.raises(dsm.DsmError, match="dsm error -1"):
        eng.debug_text_pick(crafted, np.zeros((1, 4), dtype=np.float32), [0])       # the set names token 4
    with pytest.raises(dsm.DsmError, match="dsm error -1"):
        eng.debug_text_pick(crafted, np.zeros((1, 64), dtype=np.float32), [6])      # nodes 0 .. 5
    with pytest.raises(dsm.DsmError, match="dsm error -1"):
        eng.debug_text_pick(0, np.zeros((1, 15361), dtype=np.float32), [0])         # longer than the kernel stages
    with pytest.raises(dsm.DsmError, match="dsm error -1"):
        eng.debug_text_pick(0, np.zeros((1, 64), dtype=np.float32), [0], 0.5)       # temperature > 0 without keys
    eng.close()


def probe(dsm, cfg, weights, B, steps, mask, pcm):
    """An unbiased engine on the audio: its tokens [steps][B], the largest |logit| it met, and for every active (step, slot)
    how far the better of tokens 0 / 3 lies below the row's maximum."""
    V = cfg.text_out_vocab_size
    eng = dsm.AsrEngine(cfg, B, *weights)
    act = mask.astype(bool)
    toks, gaps, amax = [], [], 0.0
    for s in range(steps):
        _, t, _ = eng.step_pcm(pcm[s], mask)
        logits = eng.debug_read("lm.logits", B * V).reshape(B, V)[act]
        toks.append(t.copy())
        amax = max(amax, float(np.abs(logits).max()))
        gaps += (logits.max(axis=1) - np.maximum(logits[:, 0], logits[:, 3])).tolist()
    eng.close()
    return toks, amax, gaps


def keywords_from_runs(toks, slots, V, boost, chunk):
    """The unbiased token runs of the listed slots, cut at 0 / 3 and into pieces of at most `chunk` tokens; every piece becomes
    a keyword with its LAST token swapped for its successor, so that following a keyword ends in a pick the raw row did not make."""
    kws = []
    for b in slots:
        run = []
        for t in [int(step[b]) for step in toks] + [0]:
            if t not in (0, 3):
                run.append(t)
            if run and (t in (0, 3) or len(run) == chunk):
                last = run[-1] + 1
                while last in (0, 3) or last >= V:
                    last = (last + 1) % V
                kws.append((run[:-1] + [last], boost))
                run = []
    return kws or [([5, 6, 7], boost), ([5, 8], boost)]


def run_followed(dsm, cfg, weights, B, steps, mask, chunk, attach_slots=None, two_sets=False):
    """Attach, step, and after every step compare every attached slot with the host function.  One set for all the listed slots
    (tokens 0 / 3 lifted, keywords from the unbiased runs of the active ones), or with two_sets one per slot from its own run."""
    from dsm_amd import synth
    V = cfg.text_out_vocab_size
    act = np.flatnonzero(mask)
    pcm = synth.synth_pcm(B, steps)
    toks, amax, gaps = probe(dsm, cfg, weights, B, steps, mask, pcm)
    boost = float(np.float32(4 * amax + 1))           # above any difference of two logits: at a live node an edge always wins
    b03 = float(np.float32(np.percentile(gaps, 60)))  # at a leaf or at DEAD tokens 0 / 3 win about six picks in ten
    attach_slots = list(range(B)) if attach_slots is None else attach_slots
    eng = dsm.AsrEngine(cfg, B, *weights)
    eng.set_text_bias(True)
    f = Follower(dsm, eng, V)
    for i, b in enumerate(attach_slots):
        if two_sets or i == 0:
            src = [b] if two_sets else [x for x in attach_slots if mask[x]]
            tk = [(0, b03), (3, b03 + 0.125 * i)]
            kws = keywords_from_runs(toks, src, V, boost, chunk)
            handle, table = eng.bias_create(tk, kws), dsm.text_bias_compile(tk, kws, V)
        f.attach(b, handle, table)
    for s in range(steps):
        _, t, _ = eng.step_pcm(pcm[s], mask)
        f.check(s, t, set(act.tolist()))
    m = eng.metrics()
    assert m.capture_failures == 0
    return eng, f, m


@pytest.mark.parametrize("model", ["tiny", "medium_bx3"])
def test_biased_picks_inside_the_step(gpu, dsm, lib, tiny_weights, model):
    """tiny (V = 64) at B = 3 with slot 1 masked out for 14 steps — the ring of 12 wraps, the step settles into its graph — and a
    medium model (V = 256, dot_mode 1) at B = 5 for 6 steps.  Every slot is attached to one set: tokens 0 and 3 lifted, keywords
    cut from what an unbiased engine emitted on the same audio with the last piece swapped, boosted above any logit difference.
    After every step each active slot's token and node are the host function's on that step's logits row and the previous node;
    the masked slot's node stays at the root.  The run must have walked the trie, left it and come back."""
    from dsm_amd import synth
    if model == "tiny":
        cfg, weights, B, steps, mask, chunk = dsm.config_tiny(), tiny_weights, 3, 14, np.array([1, 0, 1], dtype=np.uint8), 3
    else:
        cfg = dsm.config_medium()
        cfg.dot_mode = 1
        weights = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="medium_bf16_hd128_ctx300")
        B, steps, mask, chunk = 5, 6, np.ones(5, dtype=np.uint8), 2
    eng, f, m = run_followed(dsm, cfg, weights, B, steps, mask, chunk)
    assert len(eng.stream_groups()) == 1
    print(f"{model}: returns {f.returns}, live non-root steps {f.live}, DEAD steps {f.dead}, picks != raw arg-max {f.differs}")
    assert f.returns >= 3 and f.live >= 3 and f.dead >= 1 and f.differs >= 3, (f.returns, f.live, f.dead, f.differs)
    assert m.graph_launches > 0 or steps < 4
    if model == "tiny":
        assert eng.bias_state(1)[1] == 0
    eng.close()


def test_biased_picks_with_several_stream_groups(gpu, dsm, lib, tiny_weights):
    """B = 130 splits into two stream groups (80 + 50 slots), each with a launch of its own over its rows and its slice of the
    per-slot set and node arrays: one attached slot in each group — the last of the first, the second of the second — on
    different sets, for the 14 steps of the one-group run; everyone else unattached.  The same comparison after every step and
    the same four counts over the run; and each of the two slots for itself must have walked the trie, been DEAD and been steered."""
    cfg = dsm.config_tiny()
    B = 130
    probe_eng = dsm.AsrEngine(cfg, B, *tiny_weights)
    groups = probe_eng.stream_groups()
    probe_eng.close()
    assert len(groups) >= 2 and sum(n for _, n in groups) == B
    slots = [groups[0][0] + groups[0][1] - 1, groups[1][0] + 1]
    eng, f, _ = run_followed(dsm, cfg, tiny_weights, B, 14, np.ones(B, dtype=np.uint8), 3, attach_slots=slots, two_sets=True)
    assert eng.stream_groups() == groups
    assert eng.bias_state(slots[0])[0] != eng.bias_state(slots[1])[0] and eng.bias_state(0) == (0, DEAD)
    print(f"two groups: returns {f.returns}, live non-root steps {f.live}, DEAD steps {f.dead}, picks != raw arg-max {f.differs}; "
          f"per slot [returns, live, DEAD, differs] {f.per_slot}")
    assert f.returns >= 3 and f.live >= 3 and f.dead >= 1 and f.differs >= 3, (f.returns, f.live, f.dead, f.differs)
    for b in slots:  # each group's slot walked the trie, left it, and was steered: neither sat at the root or at DEAD throughout
        _, live, dead, differs = f.per_slot[b]
        assert live >= 1 and dead >= 1 and differs >= 1, (b, f.per_slot[b])
    eng.close()


def test_biased_sampled_picks_inside_the_step(gpu, dsm, lib, orc, tiny_weights):
    """temperature 0.7: the Gumbel draw over the biased row, with the slot's stream position advancing as lm_gumbel_kernel's."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    cfg.temperature = 0.7
    B, V, steps = 3, cfg.text_out_vocab_size, 8
    eng = dsm.AsrEngine(cfg, B, *tiny_weights)
    eng.set_text_bias(True)
    tk, kws = [(0, 1.0), (3, 1.0), (9, -np.inf)], [([5, 6, 7], 30.0), ([5, 8], 30.0), ([11], 30.0)]
    handle, table = eng.bias_create(tk, kws), dsm.text_bias_compile(tk, kws, V)
    f = Follower(dsm, eng, V, 0.7)
    for b in range(B):
        eng.set_seed(b, 4100 + b)
        f.key[b], f.pos[b] = seed_key(orc, 4100 + b), 0
        f.attach(b, handle, table)
    pcm = synth.synth_pcm(B, steps)
    mask = np.array([1, 1, 0], dtype=np.uint8)
    for s in range(steps):
        _, t, _ = eng.step_pcm(pcm[s], mask)
        assert 9 not in t[:2].tolist()
        f.check(s, t, {0, 1})
    assert f.live >= 2 and eng.metrics().capture_failures == 0
    eng.close()


@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_on_with_nothing_attached_is_off(gpu, dsm, lib, tiny_weights, temperature):
    """Two engines on the same audio, one with the switch on (a set exists, no slot is attached; slot 2 is attached to an EMPTY
    set): tokens, VAD values, messages, token scores with eight alternatives and the exported slot blobs are the same."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    cfg.temperature = temperature
    B, steps = 3, 14
    on, off = dsm.AsrEngine(cfg, B, *tiny_weights), dsm.AsrEngine(cfg, B, *tiny_weights)
    for e in (on, off):
        e.set_token_scores(8)
        for b in range(B):
            e.set_seed(b, 77 + b)
    on.set_text_bias(True)
    on.bias_create(*R.crafted_set())
    on.set_bias(2, on.bias_create())
    pcm = synth.synth_pcm(B, steps)
    for s in range(steps):
        mask = np.array([1, s % 3 != 1, 1], dtype=np.uint8)
        act = mask.astype(bool)
        c1, t1, p1 = on.step_pcm(pcm[s], mask)
        c0, t0, p0 = off.step_pcm(pcm[s], mask)
        assert np.array_equal(t1[act], t0[act]) and np.array_equal(c1[act], c0[act]), s
        assert np.array_equal(bits(p1[:, act]), bits(p0[:, act])), s
        assert on.poll_msgs() == off.poll_msgs(), s
        for a, b in zip(on.token_scores(), off.token_scores()):
            assert np.array_equal(a[act].view(np.uint32), b[act].view(np.uint32)), s
    assert on.export_slots([0, 1, 2]) == off.export_slots([0, 1, 2])
    assert on.metrics().capture_failures == 0 and on.metrics().graph_launches > 0
    # off again mid-stream, then on: still the same stream (every change settles the graph anew)
    for s, flag in enumerate((False, False, False, True, True, True)):
        if s % 3 == 0:
            on.set_text_bias(flag)
        mask = np.ones(B, dtype=np.uint8)
        _, t1, p1 = on.step_pcm(pcm[s], mask)
        _, t0, p0 = off.step_pcm(pcm[s], mask)
        assert np.array_equal(t1, t0) and np.array_equal(bits(p1), bits(p0)), s
    on.close()
    off.close()


def test_token_scores_stay_those_of_the_raw_row(gpu, dsm, lib, tiny_weights):
    """Scores on and bias on: logprob and the alternatives are token_scores_host of the RAW logits row with the BIASED token."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    B, V, steps = 3, cfg.text_out_vocab_size, 8
    eng = dsm.AsrEngine(cfg, B, *tiny_weights)
    eng.set_token_scores(8)
    eng.set_text_bias(True)
    handle = eng.bias_create([(0, 0.5), (3, 0.5)], [([5, 6, 7], 40.0), ([9], 40.0), ([5, 6, 12], 40.0)])
    for b in range(B):
        eng.set_bias(b, handle)
    pcm = synth.synth_pcm(B, steps)
    mask = np.ones(B, dtype=np.uint8)
    differs = 0
    for s in range(steps):
        _, t, _ = eng.step_pcm(pcm[s], mask)
        logits = eng.debug_read("lm.logits", B * V).reshape(B, V)
        lp, ids, lps = eng.token_scores()
        for b in range(B):
            h_lp, h_ids, h_lps = dsm.token_scores_host(logits[b], t[b], 8)
            assert bits(lp[b]) == bits(h_lp) and np.array_equal(ids[b], h_ids) and np.array_equal(bits(lps[b]), bits(h_lps)), (s, b)
            assert ids[b, 0] == R.first_max(logits[b])
            differs += int(ids[b, 0] != t[b])
    assert differs >= 3, differs
    eng.close()


def test_sets_attachments_resets_and_snapshots(gpu, dsm, lib, tiny_weights):
    cfg = dsm.config_tiny()
    V = cfg.text_out_vocab_size
    ones3 = np.ones(3, dtype=np.uint8)
    codes = random_codes(cfg, 3, 30, seed=1)
    A = dsm.AsrEngine(cfg, 3, *tiny_weights)
    assert A.bias_state(0) == (0, DEAD)
    # ---- handles and references ----
    tk, kws = [(0, 60.0), (3, 60.0)], [([5, 6], 30.0)]
    s1, s2 = A.bias_create(tk, kws), A.bias_create(*R.crafted_set())
    assert (s1, s2) == (1, 2) and A.bias_info(s1)["refs"] == 0
    A.set_bias(0, s1)   # works with the switch off
    A.set_bias(1, s1)
    assert A.bias_info(s1)["refs"] == 2 and A.bias_state(1) == (s1, 0)
    A.set_bias(1, s2)
    assert A.bias_info(s1)["refs"] == 1 and A.bias_info(s2)["refs"] == 1
    with pytest.raises(dsm.DsmError, match=r"dsm error -4: .*in use by 1 slots"):
        A.bias_destroy(s1)
    A.set_bias(0, 0)
    A.bias_destroy(s1)
    for call in (lambda: A.bias_info(s1), lambda: A.set_bias(0, s1), lambda: A.bias_destroy(s1), lambda: A.set_bias(3, s2),
                 lambda: A.bias_destroy(0)):
        with pytest.raises(dsm.DsmError, match="dsm error -1"):
            call()
    s3 = A.bias_create(tk, kws)
    assert s3 == 3 and A.bias_state(0) == (0, DEAD)   # never reused
    # ---- refusals of create: the engine stays as it was ----
    for bad_tokens, bad_kws in (([(V, 1.0)], []), ([(5, float("inf"))], []), ([(5, float("nan"))], []), ([(5, 1.0), (5, 1.0)], []),
                                ([], [([], 1.0)]), ([], [([5] * 33, 1.0)]), ([], [([V], 1.0)]), ([], [([0], 1.0)]), ([], [([5, 3], 1.0)]),
                                ([], [([5], 0.0)]), ([], [([5], float("inf"))]), ([(t % 64, 1.0) for t in range(1025)], [])):
        with pytest.raises(dsm.DsmError, match="dsm error -1: text bias"):
            A.bias_create(bad_tokens, bad_kws)
    assert A.bias_create() == 4
    # ---- words as text ----
    tok = dsm.Tokenizer(SPM_MODEL)
    words = ["engine", "frames", "the"]
    st = A.bias_create_text(tok, words, [2.0, 3.0, 4.0], [(7, -1.0)])
    want = dsm.text_bias_compile([(7, -1.0)], [(tok.encode(w), b) for w, b in zip(words, (2.0, 3.0, 4.0))], V)
    assert A.bias_info(st) == dict(nodes=int(want[4]), edges=int(want[5]), tokens=1, refs=0, device_bytes=4 * want.size)
    for bad, what in ((["engine", "a b"], "word 1 contains whitespace"), (["fra\tmes"], "word 0 contains whitespace"), ([""], "word 0 encodes to nothing"),
                      (["the", "the", "z" * 40], "word 2 encodes to 41 pieces"), (["Q"], "word 0 yields piece 0")):
        with pytest.raises(dsm.DsmError, match="dsm error -1: text bias: " + what):
            A.bias_create_text(tok, bad, [1.0] * len(bad))
    small_cfg, small_w = resized_tiny(dsm, 40)
    small = dsm.AsrEngine(small_cfg, 1, *small_w)
    with pytest.raises(dsm.DsmError, match="dsm error -1: text bias: word 0 yields piece 41"):
        small.bias_create_text(tok, ["x"], [1.0])
    small.close()
    # ---- a reset keeps the set and returns the node to the root; an attach in mid-stream is DEAD until the next 0 / 3 ----
    A.set_text_bias(True)
    t3 = dsm.text_bias_compile(tk, kws, V)
    f = Follower(dsm, A, V)
    f.attach(0, s3, t3)
    for s in range(3):
        text, _ = A.step_tokens(codes[s], ones3)
        f.check(s, text, {0, 1, 2})
    f.attach(2, s3, t3, node=DEAD)   # slot 2 has stepped three times
    healed = None
    for s in range(3, 8):
        text, _ = A.step_tokens(codes[s], ones3)
        f.check(s, text, {0, 1, 2})
        if healed is None and f.node[2] == 0:
            healed = s
    assert healed is not None and f.dead >= 1, "tokens 0 / 3 are lifted by 60: the slot heals at its first free pick"
    A.reset_batch_idx(2)
    assert A.bias_state(2) == (s3, 0)
    f.node[2] = 0
    text, _ = A.step_tokens(codes[8], ones3)
    f.check(8, text, {0, 1, 2})
    assert A.bias_info(s3)["refs"] == 2
    # ---- snapshots: the blob does not know the feature ----
    P, Q = dsm.AsrEngine(cfg, 3, *tiny_weights), dsm.AsrEngine(cfg, 3, *tiny_weights)
    P.set_text_bias(True)
    P.set_bias(1, P.bias_create())  # attached to an empty set: x == l
    for s in range(10):
        tp, _ = P.step_tokens(codes[s], np.array([1, 1, 0], dtype=np.uint8))
        tq, _ = Q.step_tokens(codes[s], np.array([1, 1, 0], dtype=np.uint8))
        assert np.array_equal(tp[:2], tq[:2])
    blob = P.export_slots([1])
    assert blob == Q.export_slots([1])
    fresh = P.export_slots([2])  # never stepped
    assert fresh == Q.export_slots([2])
    # import into an attached slot: its own attachment, node DEAD (root for the never-stepped slot); then the host function again
    C_ = dsm.AsrEngine(cfg, 2, *tiny_weights)
    C_.set_text_bias(True)
    hc = C_.bias_create(tk, kws)
    g = Follower(dsm, C_, V)
    g.attach(0, hc, t3)
    g.attach(1, hc, t3)
    C_.import_slots([0], blob)
    assert C_.bias_state(0) == (hc, DEAD) and C_.bias_state(1) == (hc, 0)
    C_.import_slots([1], fresh)
    assert C_.bias_state(1) == (hc, 0)
    g.node[0] = DEAD
    other = random_codes(cfg, 1, 8, seed=2000)
    for s in range(10, 18):
        text, _ = C_.step_tokens(np.stack([codes[s][1], other[s - 10][0]]), np.ones(2, dtype=np.uint8))
        g.check(s, text, {0, 1})
    assert g.dead >= 1 and g.returns >= 1
    # a fork inside one engine: slot 0 (attached, somewhere in its stream) -> slot 1; slot 1 keeps its attachment, node DEAD
    before = C_.bias_state(0)
    C_.move_slots([0], C_, [1])
    assert C_.bias_state(1) == (hc, DEAD) and C_.bias_state(0) == before
    g.node[1] = DEAD
    text, _ = C_.step_tokens(np.stack([codes[18][1], codes[18][1]]), np.ones(2, dtype=np.uint8))
    g.check(18, text, {0, 1})
    for e in (A, P, Q, C_):
        assert e.metrics().capture_failures == 0
        e.close()


def test_switch_refuses_a_vocabulary_the_kernel_cannot_stage(gpu, dsm, lib):
    cfg, weights = resized_tiny(dsm, 15361)
    eng = dsm.AsrEngine(cfg, 1, *weights)
    with pytest.raises(dsm.DsmError, match="dsm error -1: text bias: text_out_vocab_size 15361"):
        eng.set_text_bias(True)
    eng.set_text_bias(False)
    eng.close()
    cfg, weights = resized_tiny(dsm, 3)  # token 3, a word terminator, does not exist
    eng = dsm.AsrEngine(cfg, 1, *weights)
    with pytest.raises(dsm.DsmError, match="dsm error -1: text bias: text_out_vocab_size 3"):
        eng.set_text_bias(True)
    eng.close()


def test_worker_biased_channel_beside_an_unbiased_one(gpu, dsm, lib, tiny_weights):
    """40 noise frames on two channels: with channel 0 attached to a set that bans what it would say, channel 1's wire bytes are
    those of a run that never heard of the feature; closing the biased channel detaches its slot."""
    cfg = dsm.config_tiny()
    B, frames = 2, 40
    rng = np.random.default_rng(12)
    audio = [(0.1 * rng.standard_normal((B, 1920))).astype(np.float32) for _ in range(frames)]

    def run(biased):
        eng = dsm.AsrEngine(cfg, B, *tiny_weights)
        w = dsm.Worker(eng)
        slots = [w.open() for _ in range(B)]
        handle = 0
        if biased:
            eng.set_text_bias(True)
            handle = eng.bias_create([(0, 3.0), (3, 3.0)], [([5, 6, 7], 40.0), ([9], 40.0)])
            w.set_bias(slots[0], handle)
            assert eng.bias_info(handle)["refs"] == 1 and eng.bias_state(slots[0]) == (handle, 0)
        raw = {s: [] for s in slots}
        buf, n = np.zeros(1 << 16, dtype=np.uint8), C.c_size_t(0)
        for fr in range(frames):
            for s in slots:
                w.send(s, dsm.encode_in_msg("Audio", pcm=audio[fr][s]))
            assert w.step()
            for s in slots:
                while lib.dsm_worker_recv(w.h, s, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == 1:
                    raw[s].append(buf[:n.value].tobytes())
        if biased:
            w.close_channel(slots[0])
            w.send(slots[1], dsm.encode_in_msg("Audio", pcm=audio[0][1]))
            assert w.step()
            assert eng.bias_info(handle)["refs"] == 0 and eng.bias_state(slots[0]) == (0, DEAD)
            with pytest.raises(dsm.DsmError, match="dsm error -4: channel is closed"):
                w.set_bias(slots[0], handle)
            # a channel still open and biased when the worker goes: the worker detaches what it attached
            w.set_bias(slots[1], handle)
            assert eng.bias_info(handle)["refs"] == 1
            w.close()
            assert eng.bias_info(handle)["refs"] == 0 and eng.bias_state(slots[1]) == (0, DEAD)
            eng.bias_destroy(handle)
        w.close()
        eng.close()
        return [raw[s] for s in slots]

    with_bias, without = run(True), run(False)
    assert with_bias[1] == without[1] and len(without[1]) > 0
    assert with_bias[0] != without[0], "the biased channel said what the unbiased one said: the set did nothing"
