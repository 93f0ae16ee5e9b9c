"""Slot snapshots on the GPU (dsm_asr_export_slots / import / move): a stream whose state was exported from one engine and
imported into another continues bit for bit — Mimi codes, text tokens, VAD probabilities, Word / EndWord messages — and the
slots around it behave as if nothing had been imported.  config_tiny wraps the LM ring (12) and the Mimi ring (10) within a
few frames and has a 24-byte conv state at a 4-byte-aligned address (the kernels' word path); config_medium has the real
head dims (the 16-byte ring path over more than one piece per section).  Floats are compared as uint32."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONT = 14  # frames after the import: both rings wrap again


def slot_msgs(msgs, slot):
    """Word / EndWord messages of one slot, without the slot number."""
    return [(m[0],) + tuple(m[2:]) for m in msgs if m[0] != "Step" and m[1] == slot]


def step(eng, pcm, mask=None):
    """One step_pcm; per slot (codes, text, VAD bits, messages)."""
    mask = np.ones(eng.B, dtype=np.uint8) if mask is None else mask
    codes, text, prs = eng.step_pcm(pcm, mask)
    msgs = eng.poll_msgs()
    return [(codes[b].copy(), int(text[b]), prs[:, b].view(np.uint32).copy(), slot_msgs(msgs, b)) for b in range(eng.B)]


def step_two_stage(eng, pcm):
    """The server's path: encode_step on the encoder side (mimi[0]), step_tokens on its device-resident codes."""
    mask = np.ones(eng.B, dtype=np.uint8)
    codes = eng.encode_step(pcm, mask)
    text, prs = eng.step_tokens(None, mask)
    msgs = eng.poll_msgs()
    return [(codes[b].copy(), int(text[b]), prs[:, b].view(np.uint32).copy(), slot_msgs(msgs, b)) for b in range(eng.B)]


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


def frames_for(pcm_a, src_slot, other, s, k):
    """Frame s for a two-slot engine: slot 0 hears A's src_slot, slot 1 the other audio."""
    return np.stack([pcm_a[s][src_slot], other[s - k][0]])


def continuation(dsm, cfg, weights, k, seed=None, warm_c=0, B_a=3):
    """A steps k frames, slot 1 is exported and imported into slot 0 of C (which stepped warm_c frames before), then both
    run CONT frames; D is C's control without the import.  Returns the number of Word messages that were compared."""
    from dsm_amd import synth
    A = dsm.AsrEngine(cfg, B_a, *weights)
    C = dsm.AsrEngine(cfg, 2, *weights)
    D = dsm.AsrEngine(cfg, 2, *weights)
    pcm = synth.synth_pcm(B_a, k + CONT)
    other = synth.synth_pcm(1, CONT, seed=2000)
    warm = synth.synth_pcm(2, max(warm_c, 1), seed=3000)
    if seed is not None:
        A.set_seed(1, seed)
    for s in range(k):
        step(A, pcm[s])
    for s in range(warm_c):
        assert all(same(x, y) for x, y in zip(step(C, warm[s]), step(D, warm[s])))
    blob = A.export_slots([1])
    info = dsm.slot_blob_info(blob)
    assert info["n_slots"] == 1 and info["total_bytes"] == len(blob)
    assert info["flags"] == (dsm.SLOT_BLOB_HAS_MODEL_MIMI if k > 0 else 0)  # the model-side Mimi exists once step_pcm ran
    C.import_slots([0], blob)
    words = 0
    for s in range(k, k + CONT):
        a = step(A, pcm[s])[1]
        c = step(C, frames_for(pcm, 1, other, s, k))
        d = step(D, frames_for(pcm, 1, other, s, k))
        assert same(c[0], a), f"k={k}: the imported stream differs from the source at frame {s}"
        assert same(c[1], d[1]), f"k={k}: the slot beside the imported one differs from a fresh engine's at frame {s}"
        words += sum(1 for m in a[3] if m[0] == "Word")
    for e in (A, C, D):
        e.close()
    return words


@pytest.mark.parametrize("kv_bf16", [1, 0])
@pytest.mark.parametrize("k", [0, 1, 3, 17])
def test_continuation_into_a_fresh_engine(gpu, dsm, lib, tiny_weights, k, kv_bf16):
    words = continuation(dsm, dsm.config_tiny(kv_bf16), tiny_weights, k)
    print(f"k={k} kv_bf16={kv_bf16}: {words} Word messages compared")


def test_continuation_of_the_noise_stream(gpu, dsm, lib, tiny_weights):
    """temperature > 0: the slot's ChaCha key and position travel with it.  With seed 4 at temperature 2 the stream draws
    token 0 at frames 2 and 8: the export after frame 4 carries a word begun at frame 3 and the stop time of frame 2, and
    the Word / EndWord of frame 8 — tokens from both sides of the move, both times — must come out of C as out of A."""
    cfg = dsm.config_tiny()
    cfg.temperature = 2.0
    words = continuation(dsm, cfg, tiny_weights, 5, seed=4)
    assert words >= 1, "the chosen seed no longer produces a word after the import: pick another"


def test_import_into_a_running_engine(gpu, dsm, lib, tiny_weights):
    """C has stepped five frames: its graphs are captured, its Mimi sides' first call is long past.  The next replay sees
    the imported state."""
    continuation(dsm, dsm.config_tiny(), tiny_weights, 3, warm_c=5)
    continuation(dsm, dsm.config_tiny(), tiny_weights, 17, warm_c=5)


def test_medium_ring_sections(gpu, dsm, lib):
    """Real head dims (128 / 64), rings of 300 and 250 frames: every ring section is several 16 KB pieces of uint4 traffic."""
    from dsm_amd import synth
    cfg = dsm.config_medium()
    weights = synth.make_synth_weights(cfg, os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"), tag="medium_bf16_hd128_ctx300")
    continuation(dsm, cfg, weights, 40, B_a=2)


def test_step_tokens_path_without_model_side_mimi(gpu, dsm, lib, tiny_weights):
    """A is driven like the server — encode_step + step_tokens — so only mimi[0] and the LM exist and its blob carries no
    model-side Mimi.  C has one (it ran step_pcm): the import resets that side of the slot, and the stream continues on C's
    encoder side, whose first call has not run yet."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    k = 5
    A = dsm.AsrEngine(cfg, 3, *tiny_weights)
    C = dsm.AsrEngine(cfg, 2, *tiny_weights)
    D = dsm.AsrEngine(cfg, 2, *tiny_weights)
    pcm = synth.synth_pcm(3, k + CONT)
    other = synth.synth_pcm(1, CONT, seed=2000)
    warm = synth.synth_pcm(2, 2, seed=3000)
    for s in range(k):
        step_two_stage(A, pcm[s])
    for s in range(2):
        step(C, warm[s])
        step(D, warm[s])
    blob = A.export_slots([1])
    assert dsm.slot_blob_info(blob)["flags"] == 0
    C.import_slots([0], blob)
    D.reset_batch_idx(0)  # what the import does to C's model-side Mimi slot 0 (and D's slot 0 is not compared)
    for s in range(k, k + CONT):
        a = step_two_stage(A, pcm[s])[1]
        c = step_two_stage(C, frames_for(pcm, 1, other, s, k))
        d = step_two_stage(D, frames_for(pcm, 1, other, s, k))
        assert same(c[0], a), f"frame {s}"
        assert same(c[1], d[1]), f"frame {s}: neighbour"
    # the model side of C's slot 0 was reset by the import: its codes (which depend on that Mimi alone) now equal those of
    # D's slot 0, reset at the same point
    for s in range(2):
        c, d = step(C, warm[s]), step(D, warm[s])
        assert np.array_equal(c[0][0], d[0][0]) and np.array_equal(c[1][0], d[1][0]), f"model-side Mimi after the import, frame {s}"
    for e in (A, C, D):
        e.close()


def test_blob_with_model_side_mimi_into_an_engine_without(gpu, dsm, lib, tiny_weights):
    """The reverse: A ran step_pcm, its blob carries the model-side Mimi; C has only been driven through encode_step +
    step_tokens and gets that side from the import."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    k = 5
    A = dsm.AsrEngine(cfg, 3, *tiny_weights)
    C = dsm.AsrEngine(cfg, 2, *tiny_weights)
    pcm = synth.synth_pcm(3, k + CONT)
    other = synth.synth_pcm(1, CONT, seed=2000)
    warm = synth.synth_pcm(2, 2, seed=3000)
    for s in range(k):
        step(A, pcm[s])
    for s in range(2):
        step_two_stage(C, warm[s])
    blob = A.export_slots([1])
    assert dsm.slot_blob_info(blob)["flags"] == dsm.SLOT_BLOB_HAS_MODEL_MIMI
    C.import_slots([0], blob)
    for s in range(k, k + CONT):
        a = step(A, pcm[s])[1]
        c = step(C, frames_for(pcm, 1, other, s, k))
        assert same(c[0], a), f"frame {s}"
    A.close()
    C.close()


def test_move_slots_equals_export_then_import(gpu, dsm, lib, tiny_weights):
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    k, n = 4, 6
    A, A2 = dsm.AsrEngine(cfg, 3, *tiny_weights), dsm.AsrEngine(cfg, 3, *tiny_weights)
    E1, E2 = dsm.AsrEngine(cfg, 2, *tiny_weights), dsm.AsrEngine(cfg, 2, *tiny_weights)
    pcm = synth.synth_pcm(3, k + n)
    for s in range(k):
        step(A, pcm[s])
        step(A2, pcm[s])
    A.move_slots([2, 0], E1, [0, 1])
    E2.import_slots([0, 1], A2.export_slots([2, 0]))
    for s in range(k, k + n):
        a = step(A, pcm[s])  # the source slots were left untouched: A simply goes on
        e1 = step(E1, pcm[s][[2, 0]])
        e2 = step(E2, pcm[s][[2, 0]])
        assert same(e1[0], e2[0]) and same(e1[1], e2[1]), f"frame {s}: move differs from export + import"
        assert same(e1[0], a[2]) and same(e1[1], a[0]), f"frame {s}: moved streams differ from the source"
    for e in (A, A2, E1, E2):
        e.close()


def test_fork_within_one_engine(gpu, dsm, lib, tiny_weights):
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    k, n = 4, 6
    A = dsm.AsrEngine(cfg, 3, *tiny_weights)
    pcm = synth.synth_pcm(3, k + n)
    for s in range(k):
        step(A, pcm[s])
    A.move_slots([0], A, [2])
    with pytest.raises(dsm.DsmError, match="both a source and a destination"):
        A.move_slots([0, 1], A, [1, 2])
    for s in range(k, k + n):
        f = pcm[s].copy()
        f[2] = f[0]
        a = step(A, f)
        assert same(a[0], a[2]), f"frame {s}: the fork differs from its origin"
    A.close()


def test_refusals_change_nothing(gpu, dsm, lib, tiny_weights):
    """Every refused call raises DsmError, and the engine it was made on then steps exactly like its control."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    A = dsm.AsrEngine(cfg, 3, *tiny_weights)
    C = dsm.AsrEngine(cfg, 2, *tiny_weights)
    D = dsm.AsrEngine(cfg, 2, *tiny_weights)
    pcm = synth.synth_pcm(3, 3)
    pcm2 = synth.synth_pcm(2, 6, seed=3000)
    for s in range(3):
        step(A, pcm[s])
    for s in range(2):
        step(C, pcm2[s])
        step(D, pcm2[s])
    blob, blob2 = A.export_slots([1]), A.export_slots([1, 2])
    info = dsm.slot_blob_info(blob)

    cfg_ctx = dsm.config_tiny()
    cfg_ctx.lm.context = 16
    other_ctx = dsm.AsrEngine(cfg_ctx, 1, *tiny_weights)
    with pytest.raises(dsm.DsmError, match="lm.context differs"):
        C.import_slots([0], other_ctx.export_slots([0]))
    other_ctx.close()
    other_kv = dsm.AsrEngine(dsm.config_tiny(kv_bf16=0), 1, *tiny_weights)
    with pytest.raises(dsm.DsmError, match="kv_bf16 differs"):
        C.import_slots([0], other_kv.export_slots([0]))
    other_kv.close()
    for cut in (len(blob) - 16, len(blob) // 2, 100, 40):
        with pytest.raises(dsm.DsmError, match="truncated|shorter"):
            C.import_slots([0], blob[:cut])
    # the LM's ring write index is the second section of the payload: 16 bytes in
    payload = info["total_bytes"] - info["slot_bytes"]
    assert struct.unpack_from("<I", blob, payload + 16)[0] == 3 % cfg.lm.context
    bad = bytearray(blob)
    struct.pack_into("<I", bad, payload + 16, cfg.lm.context)
    with pytest.raises(dsm.DsmError, match="ring index 12 >= context 12"):
        C.import_slots([0], bytes(bad))
    with pytest.raises(dsm.DsmError, match="out of range"):
        C.import_slots([2], blob)
    with pytest.raises(dsm.DsmError, match="out of range"):
        C.export_slots([-1])
    with pytest.raises(dsm.DsmError, match="listed twice"):
        C.import_slots([1, 1], blob2)
    with pytest.raises(dsm.DsmError, match="listed twice"):
        A.move_slots([0, 1], C, [0, 0])
    with pytest.raises(dsm.DsmError, match="holds 1 slots"):
        C.import_slots([0, 1], blob)
    ones = np.ones(2, dtype=np.uint8)
    tc, td = C.encode_step_async(pcm2[2], ones), D.encode_step_async(pcm2[2], ones)
    with pytest.raises(dsm.DsmError, match="ticket"):
        C.export_slots([0])
    tx, px = C.step_tokens_ticket(tc, ones)
    ty, py = D.step_tokens_ticket(td, ones)
    assert np.array_equal(tx, ty) and np.array_equal(px.view(np.uint32), py.view(np.uint32))
    for s in range(3, 6):
        assert all(same(x, y) for x, y in zip(step(C, pcm2[s]), step(D, pcm2[s]))), f"frame {s}: a refused call changed the engine"
    for e in (A, C, D):
        e.close()
