"""Text bias on the host (csrc/dsm_text_bias.h; no GPU): dsm_text_bias_compile gives the words of the Python restatement in
tests/text_bias_ref.py, refuses what the header says it refuses, and dsm_text_bias_pick_host gives the token and the node numpy
gives on crafted rows.  Floats are compared as uint32."""
import os

import numpy as np
import pytest

import text_bias_ref as R
from text_bias_ref import DEAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(dsm, tokens, keywords, V):
    got = dsm.text_bias_compile(tokens, keywords, V)
    want = R.compile_ref(tokens, keywords, V)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (got, want)
    return got


def refused(dsm, tokens, keywords, V, word):
    with pytest.raises(dsm.DsmError) as ei:
        dsm.text_bias_compile(tokens, keywords, V)
    assert ei.value.code == -1 and word in str(ei.value), str(ei.value)


def test_compile_gives_the_words_of_the_restatement(dsm, lib):
    # shared prefixes, a keyword that is a prefix of another, duplicates with different boosts: the maximum wins on every edge
    kws = [([7, 8, 9], 2.0), ([7, 8], 3.0), ([7, 5], 1.0), ([7, 8, 9], 0.5), ([6], 4.0), ([6], 4.5), ([12, 7, 8], 1.25)]
    toks = [(9, -1.0), (1, np.float32(0.1)), (63, -np.inf), (0, 2.0), (3, 2.5)]
    t = both(dsm, toks, kws, 64)
    tb, nodes = R.parse(t)
    assert [x for x, _ in tb] == [0, 1, 3, 9, 63]
    assert list(nodes[0]) == [6, 7, 12] and nodes[0][6][0] == 4.5 and nodes[0][7][0] == 3.0
    seven = nodes[nodes[0][7][1]]
    assert list(seven) == [5, 8] and seven[8][0] == 3.0 and nodes[seven[8][1]][9][0] == 2.0
    assert t[0] == R.MAGIC and t[2] == 64 and t[4] == 9 and t[5] == 8 and t[6] == t.size
    # breadth-first numbering with sorted edges: edge e leads to node e + 1
    assert np.array_equal(t[R.HEADER + 2 * 5 + 9 + 1:].reshape(8, 3)[:, 2], np.arange(1, 9))
    # a function of the SET of inputs: every permutation gives the same words
    rng = np.random.default_rng(3)
    for _ in range(6):
        k2 = [kws[i] for i in rng.permutation(len(kws))]
        t2 = [toks[i] for i in rng.permutation(len(toks))]
        assert np.array_equal(dsm.text_bias_compile(t2, k2, 64), t)
    # nothing at all: the root alone
    e = both(dsm, [], [], 64)
    assert e.tolist() == [R.MAGIC, 1, 64, 0, 1, 0, 10, 0, 0, 0]
    both(dsm, [(5, 1.0)], [], 8)
    both(dsm, [], [([5], 1.0)], 8)
    # a random larger set
    kws = [(rng.choice(np.array([1, 2] + list(range(4, 500))), size=int(rng.integers(1, 7))).tolist(), float(rng.uniform(0.1, 9))) for _ in range(400)]
    toks = [(int(t), float(v)) for t, v in zip(rng.choice(500, 100, replace=False), rng.standard_normal(100))]
    both(dsm, toks, kws, 500)
    both(dsm, [(t, 0.5) for t in range(R.MAX_TOKENS)], [([4] * R.MAX_KEYWORD_TOKENS, 1.0)], 2000)


def test_node_counts_on_both_sides_of_the_limit(dsm, lib):
    """65534 one-piece keywords are 65535 nodes with the root: allowed; one more is refused.  So is a deep trie that crosses it."""
    V = 70000
    pieces = [p for p in range(1, 65540) if p != 3]
    ok = [([p], 1.0) for p in pieces[:R.MAX_NODES - 1]]
    t = both(dsm, [], ok, V)
    assert t[4] == R.MAX_NODES and t[5] == R.MAX_NODES - 1
    refused(dsm, [], ok + [([pieces[R.MAX_NODES - 1]], 1.0)], V, "trie nodes")
    deep = [([p] + [7] * 31, 1.0) for p in pieces[:2048]]  # 2048 * 32 = 65536 nodes behind the root
    refused(dsm, [], deep, V, "trie nodes")
    t = both(dsm, [], deep[:2047] + [([pieces[2047]] + [7] * 29, 1.0)], V)  # 2047 * 32 + 30 = 65534 behind the root
    assert t[4] == R.MAX_NODES
    refused(dsm, [], deep[:2047] + [([pieces[2047]] + [7] * 30, 1.0)], V, "trie nodes")


def test_compile_refusals(dsm, lib):
    inf, nan = float("inf"), float("nan")
    refused(dsm, [(64, 1.0)], [], 64, "outside the vocabulary")
    refused(dsm, [(5, inf)], [], 64, "+inf or NaN")
    refused(dsm, [(5, nan)], [], 64, "+inf or NaN")
    refused(dsm, [(5, 1.0), (6, 1.0), (5, 2.0)], [], 64, "listed twice")
    refused(dsm, [(t % 1024, 1.0) for t in range(R.MAX_TOKENS + 1)], [], 2000, "token biases")
    refused(dsm, [], [([], 1.0)], 64, "pieces")
    refused(dsm, [], [([5] * (R.MAX_KEYWORD_TOKENS + 1), 1.0)], 64, "pieces")
    refused(dsm, [], [([5, 64], 1.0)], 64, "piece 64")
    refused(dsm, [], [([5, 0], 1.0)], 64, "terminator")
    refused(dsm, [], [([3], 1.0)], 64, "terminator")
    for boost in (0.0, -1.0, inf, -inf, nan):
        refused(dsm, [], [([5], boost)], 64, "boost")
    refused(dsm, [], [], 0, "V")
    dsm.text_bias_compile([(5, -inf), (6, -3.0e38)], [([5], 3.0e38)], 64)  # a ban, and finite values however large, are fine
    # the buffer convention: a size query, then a buffer that is too small
    import ctypes as C
    need = C.c_size_t(0)
    assert lib.dsm_text_bias_compile(None, 0, None, 0, 64, None, 0, C.byref(need)) == 0 and need.value == 10
    small = np.zeros(9, dtype=np.uint32)
    assert lib.dsm_text_bias_compile(None, 0, None, 0, 64, small.ctypes.data_as(C.c_void_p), 9, None) == -1
    assert not small.any()


def test_pick_host_on_crafted_rows(dsm, lib):
    """The crafted rows of text_bias_ref (a banned arg-max, a tie a bias creates, a token with a bias and a boost whose two adds
    do not commute, all-banned and all-NaN rows, every kind of node, every branch of the advance) at row lengths on both sides of
    256, against the numpy restatement."""
    assert R.ORDER_RIGHT.view(np.uint32) != R.ORDER_WRONG.view(np.uint32)  # the order of the two adds shows in these rows
    seen_nodes, seen_moves = set(), set()
    for V in (5, 64, 255, 256, 257, 1000):
        table = both(dsm, *R.crafted_set(), V)
        _, nodes = R.parse(table)
        for row, node in R.crafted_rows(V):
            tok, nxt = dsm.text_bias_pick_host(table, node, row)
            assert (tok, nxt) == R.pick_ref(table, node, row), (V, node)
            assert dsm.text_bias_pick_host(None, node, row) == (R.first_max(row), node)  # no set: the raw pick, the node untouched
            seen_nodes.add("dead" if node == DEAD else "root" if node == 0 else "leaf" if not nodes[node] else "inner")
            seen_moves.add("terminator" if tok in (0, 3) else "stays dead" if node == DEAD else "child" if nxt != DEAD else "no child")
    assert seen_nodes == {"dead", "root", "leaf", "inner"} and seen_moves == {"terminator", "stays dead", "child", "no child"}
    table = dsm.text_bias_compile(*R.crafted_set(), 64)
    rows = dict((i, rn) for i, rn in enumerate(R.crafted_rows(64)))
    assert dsm.text_bias_pick_host(table, 0, rows[0][0])[0] != 2 and R.first_max(rows[0][0]) == 2      # the ban
    assert dsm.text_bias_pick_host(table, 0, rows[2][0]) == (0, 0)                                     # the created tie: lower id
    assert dsm.text_bias_pick_host(table, 0, rows[3][0]) == (1, 1)
    assert dsm.text_bias_pick_host(table, 0, rows[9][0]) == (4, 2) and dsm.text_bias_pick_host(table, DEAD, rows[9][0]) == (0, 0)
    # every token banned by the set itself
    ban = dsm.text_bias_compile([(t, -np.inf) for t in range(5)], [([4], 2.0)], 5)
    assert dsm.text_bias_pick_host(ban, 0, np.arange(5, dtype=np.float32)) == (0, 0)
    # an empty set is "x == l"
    empty = dsm.text_bias_compile([], [], 64)
    for row, _ in R.crafted_rows(64):
        assert dsm.text_bias_pick_host(empty, 0, row)[0] == R.first_max(row)


def test_pick_host_with_gumbel_noise(dsm, lib, orc):
    """temperature > 0: an empty set and no set draw the same token from the same stream words; a ban is never drawn, a boost
    far above the noise always is; the draw depends on the key and on the position, 16 words apart."""
    import ctypes as C
    V = 100
    rng = np.random.default_rng(5)
    key = (C.c_uint32 * 8)()
    orc.lib().orc_seed_from_u64(77, key)
    key = np.array(list(key), dtype=np.uint32)
    empty = dsm.text_bias_compile([], [], V)
    ban = dsm.text_bias_compile([(t, -np.inf) for t in range(0, V, 2)], [], V)
    lift = dsm.text_bias_compile([(41, -50.0)], [([41], 1000.0), ([41, 17], 1000.0)], V)
    draws = set()
    for i in range(40):
        row = rng.standard_normal(V).astype(np.float32)
        pos = 16 * 7 * i
        t0, _ = dsm.text_bias_pick_host(None, 0, row, 0.8, key, pos)
        assert dsm.text_bias_pick_host(empty, 0, row, 0.8, key, pos) == (t0, 0 if t0 in (0, 3) else DEAD)
        assert dsm.text_bias_pick_host(ban, DEAD, row, 0.8, key, pos)[0] % 2 == 1
        assert dsm.text_bias_pick_host(lift, 0, row, 0.8, key, pos) == (41, 1)
        assert dsm.text_bias_pick_host(lift, 1, row, 0.8, key, pos) == (17, 2)
        assert dsm.text_bias_pick_host(lift, DEAD, row, 0.8, key, pos)[0] != 41
        assert dsm.text_bias_pick_host(None, 0, row, 1.0, key, pos)[0] < V  # the temperature == 1 branch of dsm_gumbel_value
        draws.add(t0)
    assert len(draws) > 10
    row = np.zeros(V, dtype=np.float32)
    assert len({dsm.text_bias_pick_host(None, 0, row, 0.8, key, 16 * i)[0] for i in range(30)}) > 10
    assert dsm.text_bias_pick_host(None, 0, row, 0.8, key, 0) == dsm.text_bias_pick_host(None, 0, row, 0.8, key, 0)


def test_pick_host_refusals(dsm, lib):
    table = dsm.text_bias_compile(*R.crafted_set(), 64)
    row = np.zeros(64, dtype=np.float32)
    key = np.arange(8, dtype=np.uint32)

    def bad(*a, **k):
        with pytest.raises(dsm.DsmError) as ei:
            dsm.text_bias_pick_host(*a, **k)
        assert ei.value.code == -1

    bad(table, 6, row)                       # the set has nodes 0 .. 5
    bad(table, 0, row[:4])                   # the table names token 4
    bad(table, 0, row, 0.5)                  # temperature > 0 without a key
    bad(table, 0, row, 0.5, key, 8)          # a position that is not a multiple of 16
    bad(table, 0, row, float("nan"), key)
    bad(table[:-1], 0, row)                  # truncated
    for at, value in ((0, 1), (1, 2), (3, 2000), (4, 0), (4, 7), (5, 4), (6, 1), (7, 1), (8, 9), (9, 0x7FC00000), (9, 0x7F800000),
                      (R.HEADER + 6, 1), (R.HEADER + 6 + 6, 9), (t_edge := R.HEADER + 6 + 7, 0), (t_edge, 3), (t_edge, 64),
                      (t_edge + 1, 0), (t_edge + 1, 0xBF800000), (t_edge + 1, 0x7F800000), (t_edge + 2, 2), (t_edge + 2, 0)):
        t = table.copy()
        t[at] = value
        bad(t, 0, row)
    assert dsm.text_bias_pick_host(table, 0, row) == R.pick_ref(table, 0, row)


def test_every_declared_symbol_is_exported(dsm, lib):
    for name in ("dsm_asr_set_text_bias", "dsm_asr_bias_create", "dsm_asr_bias_create_text", "dsm_asr_bias_destroy", "dsm_asr_bias_info",
                 "dsm_asr_set_bias", "dsm_asr_bias_state", "dsm_text_bias_compile", "dsm_text_bias_pick_host", "dsm_debug_text_pick",
                 "dsm_worker_set_bias"):
        assert name in dsm.ABI_SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "dsm.h")).read()
    assert "#define DSM_BIAS_MAX_TOKENS %d\n" % dsm.BIAS_MAX_TOKENS in header and "#define DSM_BIAS_MAX_NODES %d\n" % dsm.BIAS_MAX_NODES in header
    assert "#define DSM_BIAS_MAX_KEYWORD_TOKENS %d\n" % dsm.BIAS_MAX_KEYWORD_TOKENS in header and "#define DSM_BIAS_MAX_SETS %d\n" % dsm.BIAS_MAX_SETS in header


def test_worker_with_a_callers_backend_has_no_bias_sets(dsm, lib):
    """dsm_worker_set_bias on a worker built with dsm_worker_create_with_backend: DSM_ERR_STATE, whatever the slot holds."""
    import ctypes as C
    be = dsm.WorkerBackend()
    be.batch_size, be.asr_delay_in_tokens, be.extra_heads_num = 2, 2, 0
    cbs = (dsm.BE_ENCODE(lambda *_: 0), dsm.BE_RESET(lambda *_: 0), dsm.BE_STEP(lambda *_: 0), dsm.BE_POLL(lambda *_: 0))
    be.encode_step, be.reset_slot, be.step_tokens, be.poll_msgs = cbs
    w = dsm.Worker(backend=be)
    slot = w.open()
    with pytest.raises(dsm.DsmError) as ei:
        w.set_bias(slot, 1)
    assert ei.value.code == -4 and "backend" in str(ei.value)
    w.close()
