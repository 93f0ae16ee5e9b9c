"""Clips on the GPU (dsm_asr_set_clips, dsm_asr_run / dsm_asr_collect; include/dsm.h "clips"): a slot's audio lies on the device
in its own format, asr_clip_frame_kernel cuts it into frames, and a block of K steps gives — bit for bit — what a second engine
computes that is fed dsm_mimi_encode_step_raw_async + dsm_asr_step_tokens_ticket frame by frame with the rows of the independent
cut (tests/clip_ref.py) and the same masks: stepped, text tokens, VAD values, log-probabilities, the messages of every step.
Whatever the block size; with the clip pushed in pieces (the slot waits and sits steps out); beside slots that run on per-step
calls; with two stream groups; with text bias; the refusals refuse with nothing changed; a block launches the graphs of the
per-step calls and adds none.  config_tiny, B = 4 (20 for two stream groups), ten to sixteen steps.  Floats are compared as
uint32."""
import audioop

import numpy as np
import pytest

import clip_ref as R

pytestmark = pytest.mark.gpu

B, PITCH, CAP = 4, 15360, 1 << 16
# (rate, format, bytes): 3 frames + 7 samples; exactly 2 frames; 5 frames + 1 byte; nothing, closed at once
CLIPS = [(24000, R.F32, 3 * 7680 + 7 * 4), (8000, R.MULAW, 2 * 640), (11025, R.MULAW, 5 * 882 + 1), (44100, R.S16, 0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def audio_bytes(rate, fmt, n_bytes, seed):
    n = -(-n_bytes // R.SAMPLE_BYTES[fmt])
    t = np.arange(n) / rate
    rng = np.random.RandomState(17 + seed)
    x = 0.3 * np.sin(2 * np.pi * (170 + 40 * seed) * t) + 0.05 * (2 * rng.random_sample(n) - 1)
    if fmt == R.F32:
        raw = x.astype("<f4").tobytes()
    else:
        s16 = np.round(x * 32767).astype("<i2").tobytes()
        raw = s16 if fmt == R.S16 else (audioop.lin2ulaw if fmt == R.MULAW else audioop.lin2alaw)(s16, 2)
    return raw[:n_bytes]


def clips_for(slots):
    """{slot: (rate, fmt, data)}: the four clips on the given slots"""
    return {b: (rate, fmt, audio_bytes(rate, fmt, n, i)) for i, (b, (rate, fmt, n)) in enumerate(zip(slots, CLIPS))}


def flush_of(dsm):
    return dsm.config_tiny().asr_delay_in_tokens + 2


def clip_engine(dsm, tiny_weights, batch=B, scores=True):
    eng = dsm.AsrEngine(dsm.config_tiny(), batch, *tiny_weights, device_id=0)
    eng.set_clips(True, CAP)
    if scores:
        eng.set_token_scores(0)
    return eng


def begin_closed(eng, clips, flush):
    for b, (rate, fmt, data) in clips.items():
        eng.clip_begin(b, rate, fmt, flush)
        eng.clip_push(b, data)
        eng.clip_close(b)


def steps_of(blk):
    return [dict(stepped=blk.stepped[k].copy(), text=blk.text_token[k].copy(), prs=blk.vad_prs[k].copy(), lp=blk.logprob[k].copy(),
                 msgs=blk.msgs[k], scores=[(b, bits(s).tolist()) for b, s in blk.word_scores[k]]) for k in range(blk.n_steps)]


def run_until_done(eng, slots, K, limit=48):
    out = []
    while any(eng.clip_status(b) != R.DONE for b in slots):
        eng.run(K)
        out += steps_of(eng.collect())
        assert len(out) <= limit, "the clips do not end"
    return out


def plain_steps(dsm, tiny_weights, clips, table, batch=B, prepare=None):
    """the comparison engine: per step the rows of the reference cut and the step's masks through encode_step_raw_async +
    step_tokens_ticket.  table: (frame [n][batch], mask [n][batch]) of the reference schedule."""
    eng = dsm.AsrEngine(dsm.config_tiny(), batch, *tiny_weights, device_id=0)
    out = []
    try:
        eng.set_ingest(True)
        eng.set_token_scores(0)
        for b, (rate, fmt, _) in clips.items():
            eng.set_input_format(b, rate, fmt)
        if prepare:
            prepare(eng)
        frame, mask = table
        for k in range(len(mask)):
            rows = [R.frame(clips[b][2], clips[b][0], clips[b][1], int(frame[k, b])) if mask[k, b] else None for b in range(batch)]
            text, prs = eng.step_tokens_ticket(eng.encode_step_raw_async(rows, mask[k], PITCH), mask[k])
            out.append(dict(stepped=mask[k].copy(), text=text, prs=prs, lp=eng.token_scores()[0], msgs=eng.poll_msgs(),
                            scores=[(b, bits(s).tolist()) for b, s in eng.word_scores()]))
    finally:
        eng.close()
    return out


def closed_table(dsm, clips, n_steps, batch=B):
    ref = R.Schedule(batch, CAP)
    for b, (rate, fmt, data) in clips.items():
        ref.begin(b, rate, fmt, flush_of(dsm))
        ref.push(b, len(data))
        ref.close(b)
    frame, mask = zip(*[ref.run(1) for _ in range(n_steps)])
    return np.concatenate(frame), np.concatenate(mask)


def same_steps(got, want):
    """step by step; `got` may be longer by steps in which nothing stepped (a last block that outlives the clips)"""
    assert len(got) >= len(want)
    for k, g in enumerate(got):
        if k >= len(want):
            assert not g["stepped"].any() and all(m[0] == "Step" for m in g["msgs"]), k
            continue
        w = want[k]
        act = w["stepped"].astype(bool)
        assert np.array_equal(g["stepped"], w["stepped"]), (k, g["stepped"], w["stepped"])
        assert np.array_equal(g["text"][act], w["text"][act]), (k, "text tokens")
        assert np.array_equal(bits(g["prs"])[:, act], bits(w["prs"])[:, act]), (k, "VAD values")
        assert np.array_equal(bits(g["lp"])[act], bits(w["lp"])[act]), (k, "log-probabilities")
        assert g["msgs"] == w["msgs"], (k, g["msgs"], w["msgs"])
        assert g["scores"] == w["scores"], (k, "word scores")


def by_slot(steps, b):
    """what slot b saw, in its own time: the results of the steps it took, and its Word / EndWord messages"""
    took = [(int(s["text"][b]), bits(s["prs"])[:, b].tolist(), int(bits(s["lp"])[b])) for s in steps if s["stepped"][b]]
    msgs = [m for s in steps for m in s["msgs"] if m[0] != "Step" and m[1] == b]
    return took, msgs


N_STEPS = 10  # the longest clip: 6 frames of audio + 4 of flush


@pytest.fixture(scope="module")
def clips():
    return clips_for(range(B))


@pytest.fixture(scope="module")
def plain(gpu, dsm, lib, tiny_weights, clips):
    table = closed_table(dsm, clips, N_STEPS)
    assert table[1].sum(axis=0).tolist() == [4 + flush_of(dsm), 2 + flush_of(dsm), 6 + flush_of(dsm), flush_of(dsm)]
    return plain_steps(dsm, tiny_weights, clips, table)


@pytest.fixture(scope="module")
def one_push(gpu, dsm, lib, tiny_weights, clips):
    eng = clip_engine(dsm, tiny_weights)
    try:
        begin_closed(eng, clips, flush_of(dsm))
        return run_until_done(eng, range(B), 16)
    finally:
        eng.close()


def test_a_block_equals_the_per_step_calls(gpu, dsm, lib, tiny_weights, clips, plain, one_push):
    assert len(one_push) == 16
    same_steps(one_push, plain)
    assert not any(np.isnan(s["lp"][s["stepped"].astype(bool)]).any() for s in one_push)


def test_the_cut_frame_reaches_mimi_as_the_host_function_gives_it(gpu, dsm, lib, tiny_weights, clips):
    eng = clip_engine(dsm, tiny_weights)
    try:
        begin_closed(eng, clips, flush_of(dsm))
        for k in range(2):  # frame 0, then frame 1 (slot 3: silence both times)
            eng.run(1)
            blk = eng.collect()
            assert blk.n_steps == 1 and blk.stepped[0].tolist() == [1, 1, 1, 1]
            got = eng.debug_ingest_read(0)
            for b, (rate, fmt, data) in clips.items():
                host = dsm.ingest_host(rate, fmt)
                for i in range(k + 1):
                    want = host.step(dsm.asr_clip_frame_host(data, rate, fmt, i))
                assert np.array_equal(bits(got[b]), bits(want)), (k, b)
    finally:
        eng.close()


@pytest.mark.parametrize("K", [1, 3])
def test_block_size_does_not_matter(gpu, dsm, lib, tiny_weights, clips, plain, one_push, K):
    eng = clip_engine(dsm, tiny_weights)
    try:
        begin_closed(eng, clips, flush_of(dsm))
        got = run_until_done(eng, range(B), K)
        assert len(got) == -(-N_STEPS // K) * K
        same_steps(got, plain)
        same_steps(one_push, got)
        assert [eng.clip_status(b) for b in range(B)] == [R.DONE] * B
    finally:
        eng.close()


def test_a_clip_pushed_in_pieces_waits_and_gives_the_same(gpu, dsm, lib, tiny_weights, clips, one_push):
    flush = flush_of(dsm)
    eng = clip_engine(dsm, tiny_weights)
    ref = R.Schedule(B, CAP)
    try:
        for b, (rate, fmt, data) in clips.items():
            eng.clip_begin(b, rate, fmt, flush); ref.begin(b, rate, fmt, flush)
            part = data[:len(data) // 2] if b in (0, 2) else data  # slots 0 and 2: half now (in the middle of a frame)
            eng.clip_push(b, part); ref.push(b, len(part))
            if b not in (0, 2):
                eng.clip_close(b); ref.close(b)
        eng.run(3)
        got = steps_of(eng.collect())
        _, mask = ref.run(3)
        assert np.array_equal(np.stack([s["stepped"] for s in got]), mask)
        assert mask[:, 0].tolist() == [1, 0, 0] and mask[:, 2].tolist() == [1, 1, 0]  # 1.5 and 2.5 frames were there
        assert eng.clip_status(0) == R.WAITING and eng.clip_status(2) == R.WAITING and eng.clip_status(1) == R.RUNNING
        eng.run(1)  # nothing pushed: they sit this one out too
        got += steps_of(eng.collect())
        assert got[-1]["stepped"].tolist() == [0, 1, 0, 1]
        for b in (0, 2):
            data = clips[b][2]
            eng.clip_push(b, data[len(data) // 2:])
            assert eng.clip_status(b) == R.RUNNING
            eng.clip_close(b)
        got += run_until_done(eng, range(B), 5)
        for b in range(B):
            assert by_slot(got, b) == by_slot(one_push, b), b
        for s in got:  # a step sat out delivers nothing for the slot
            assert all(m[0] == "Step" or s["stepped"][m[1]] for m in s["msgs"])
    finally:
        eng.close()


def test_clip_slots_and_per_step_slots_side_by_side(gpu, dsm, lib, tiny_weights, clips, one_push):
    """slots 0-1 run clips, slots 2-3 run on dsm_asr_step_raw between blocks; each pair equals itself run alone"""
    flush = flush_of(dsm)
    two = {b: clips[b] for b in (0, 1)}
    live = np.array([0, 0, 1, 1], dtype=np.uint8)
    frames = [[None, None] + [audio_bytes(24000, R.F32, 7680, 50 + 10 * s + b) for b in (2, 3)] for s in range(4)]

    def live_step(eng, s):
        codes, text, prs = eng.step_raw(frames[s], live, 7680)
        return (codes[2:].tolist(), text[2:].tolist(), bits(prs)[:, 2:].tolist(),
                [m for m in eng.poll_msgs() if m[0] != "Step"])

    alone = clip_engine(dsm, tiny_weights)
    both = clip_engine(dsm, tiny_weights)
    try:
        want_live = [live_step(alone, s) for s in range(4)]
        begin_closed(both, two, flush)
        got_live, got = [], []
        for s in range(4):
            both.run(2)
            got += steps_of(both.collect())
            if s == 1:  # a mask bit on a clip slot: refused, nothing changed
                with pytest.raises(dsm.DsmError, match="has a clip"):
                    both.step_raw(frames[s], np.array([1, 0, 1, 1], dtype=np.uint8), 7680)
                with pytest.raises(dsm.DsmError, match="has a clip"):
                    both.encode_step_raw_async(frames[s], np.array([0, 1, 0, 0], dtype=np.uint8), 7680)
            got_live.append(live_step(both, s))
        assert got_live == want_live
        assert [both.clip_status(b) for b in range(B)] == [R.DONE, R.DONE, R.IDLE, R.IDLE]
        for b in (0, 1):
            assert by_slot(got, b) == by_slot(one_push, b), b
        for s in got:
            assert s["stepped"][2:].tolist() == [0, 0]
    finally:
        alone.close()
        both.close()


def test_two_stream_groups(gpu, dsm, lib, tiny_weights, monkeypatch):
    """the record launch of a group rides that group's stream: slots of both groups, blocks of 3"""
    monkeypatch.setenv("DSM_LM_GROUPS", "2")
    big, slots = 20, (0, 15, 16, 19)
    clips = clips_for(slots)
    want = plain_steps(dsm, tiny_weights, clips, closed_table(dsm, clips, N_STEPS, big), big)
    eng = clip_engine(dsm, tiny_weights, big)
    try:
        first, count = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
        n = eng.lib.dsm_lm_stream_groups(eng.h, first.ctypes.data_as(dsm.C.POINTER(dsm.C.c_int)), count.ctypes.data_as(dsm.C.POINTER(dsm.C.c_int)), 4)
        assert n == 2 and count[:2].tolist() == [16, 4]
        begin_closed(eng, clips, flush_of(dsm))
        same_steps(run_until_done(eng, slots, 3), want)
    finally:
        eng.close()


def test_text_bias_on_one_slot(gpu, dsm, lib, tiny_weights, clips):
    def prepare(eng):
        eng.set_text_bias(True)
        eng.set_bias(2, eng.bias_create(tokens=[(5, 6.0), (9, 6.0), (3, -float("inf"))]))

    want = plain_steps(dsm, tiny_weights, clips, closed_table(dsm, clips, N_STEPS), prepare=prepare)
    eng = clip_engine(dsm, tiny_weights)
    try:
        prepare(eng)
        begin_closed(eng, clips, flush_of(dsm))
        got = run_until_done(eng, range(B), 4)
        same_steps(got, want)
        assert not any(s["text"][2] == 3 for s in got if s["stepped"][2])  # the ban held
    finally:
        eng.close()


def test_refusals_change_nothing(gpu, dsm, lib, tiny_weights, clips, plain):
    flush = flush_of(dsm)
    off = dsm.AsrEngine(dsm.config_tiny(), B, *tiny_weights, device_id=0)
    eng = clip_engine(dsm, tiny_weights)
    try:
        for call in (lambda: off.run(1), lambda: off.collect(), lambda: off.clip_begin(0, 8000, R.MULAW, 0), lambda: off.clip_push(0, b"x")):
            with pytest.raises(dsm.DsmError, match="clips are off"):
                call()
        assert off.clip_status(0) == R.IDLE
        with pytest.raises(dsm.DsmError, match="no block waits"):
            eng.collect()
        with pytest.raises(dsm.DsmError, match="whole number"):
            eng.clip_begin(0, 8001, R.F32, 0)
        with pytest.raises(dsm.DsmError, match="negative"):
            eng.clip_begin(0, 8000, R.F32, -1)
        with pytest.raises(dsm.DsmError, match="no clip"):
            eng.clip_push(0, b"abc")
        begin_closed(eng, {b: clips[b] for b in (1, 2, 3)}, flush)
        rate, fmt, data = clips[0]
        eng.clip_begin(0, rate, fmt, flush)
        with pytest.raises(dsm.DsmError, match="has a clip"):
            eng.clip_begin(0, rate, fmt, flush)  # busy
        with pytest.raises(dsm.DsmError, match="pass the"):
            eng.clip_push(0, bytes(CAP + 1))     # past the cap
        eng.clip_push(0, data[:100])
        with pytest.raises(dsm.DsmError, match="pass the"):
            eng.clip_push(0, bytes(CAP - 99))
        eng.clip_push(0, data[100:])
        eng.clip_close(0)
        with pytest.raises(dsm.DsmError, match="closed"):
            eng.clip_push(0, b"abc")
        with pytest.raises(dsm.DsmError, match="has a clip"):
            eng.export_slots([0])
        for n in (0, 17):
            with pytest.raises(dsm.DsmError, match="n_steps"):
                eng.run(n)
        eng.run(4)
        ones = np.ones(B, dtype=np.uint8)
        for call in (lambda: eng.run(1), lambda: eng.clip_push(0, b"a"), lambda: eng.reset_batch_idx(1), lambda: eng.mimi_reset_batch_idx(1),
                     lambda: eng.step_pcm(np.zeros((B, 1920), dtype=np.float32), 0 * ones), lambda: eng.clip_begin(1, 8000, R.MULAW, 0),
                     lambda: eng.encode_step(np.zeros((B, 1920), dtype=np.float32), 0 * ones)):
            with pytest.raises(dsm.DsmError, match="waits for dsm_asr_collect"):
                call()
        got = steps_of(eng.collect())
        got += run_until_done(eng, range(B), 4)
        same_steps(got, plain)  # the blocks around the refusals are what they are without them
        eng.reset_batch_idx(0)
        assert eng.clip_status(0) == R.IDLE and eng.clip_status(1) == R.DONE
    finally:
        off.close()
        eng.close()


def test_a_block_replays_the_per_step_graphs(gpu, dsm, lib, tiny_weights, clips):
    eng = clip_engine(dsm, tiny_weights)
    try:
        live = np.array([0, 0, 0, 1], dtype=np.uint8)
        frame = [None, None, None, audio_bytes(24000, R.F32, 7680, 3)]
        begin_closed(eng, {b: clips[b] for b in (0, 1, 2)}, 12)
        for _ in range(3):
            eng.run(2)
            eng.collect()
        # the model side's encode settles too — behind the blocks, whose first encode grew the encoder stream's split-K
        # workspace, which makes every graph of the engine settle again (as the first dsm_mimi_encode_step_raw_async does)
        for _ in range(3):
            eng.step_raw(frame, live, 7680)
        m0 = eng.metrics()
        eng.run(2)
        eng.collect()
        m1 = eng.metrics()
        assert m1.graph_launches - m0.graph_launches == 2 * 2  # per step: the encode and the one group's LM step
        assert m1.eager_bodies == m0.eager_bodies and m1.capture_failures == 0
        eng.step_raw(frame, live, 7680)
        m2 = eng.metrics()
        assert m2.graph_launches - m1.graph_launches == 2 and m2.eager_bodies == m1.eager_bodies and m2.capture_failures == 0
    finally:
        eng.close()
