"""A Python restatement of csrc/dsm_text_bias.h for the tests: the flat table of a bias set, the pick of one row and the advance
of the trie node, written from the header's text with dicts and numpy — no code shared with the library.  Also the crafted rows
both the CPU and the GPU test use."""
import struct

import numpy as np

MAGIC, VERSION, HEADER = 0x54425344, 1, 8
DEAD = 0xFFFFFFFF
MAX_TOKENS, MAX_KEYWORD_TOKENS, MAX_NODES = 1024, 32, 65535


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def compile_ref(tokens, keywords, V):
    """tokens: (token, bias) pairs; keywords: (piece ids, boost) pairs -> the table as a uint32 array."""
    trie = [{}]  # node -> {token: [boost, child]} in insertion order
    for ids, boost in keywords:
        at = 0
        for t in ids:
            edge = trie[at].get(int(t))
            if edge is None:
                edge = trie[at][int(t)] = [np.float32(boost), len(trie)]
                trie.append({})
            elif np.float32(boost) > edge[0]:
                edge[0] = np.float32(boost)
            at = edge[1]
    order = [0]  # breadth first, a node's children by ascending token
    for old in order:
        order.extend(trie[old][t][1] for t in sorted(trie[old]))
    new_of = {old: new for new, old in enumerate(order)}
    words = [MAGIC, VERSION, V, len(tokens), len(trie), len(trie) - 1, 0, 0]
    for t, v in sorted((int(t), f32_bits(v)) for t, v in tokens):
        words += [t, v]
    first, edges = [0], []
    for old in order:
        for t in sorted(trie[old]):
            boost, child = trie[old][t]
            edges += [t, f32_bits(boost), new_of[child]]
        first.append(len(edges) // 3)
    words += first + edges
    words[6] = len(words)
    return np.array(words, dtype=np.uint32)


def parse(table):
    """table -> (token biases [(token, f32)], per node a dict token -> (f32 boost, child))."""
    t = np.asarray(table, dtype=np.uint32)
    nt, nn, ne = int(t[3]), int(t[4]), int(t[5])
    tb = [(int(t[HEADER + 2 * i]), t[HEADER + 2 * i + 1:HEADER + 2 * i + 2].view(np.float32)[0]) for i in range(nt)]
    first = t[HEADER + 2 * nt:HEADER + 2 * nt + nn + 1]
    ed = t[HEADER + 2 * nt + nn + 1:].reshape(ne, 3)
    nodes = [{int(ed[e, 0]): (ed[e, 1:2].view(np.float32)[0], int(ed[e, 2])) for e in range(int(first[n]), int(first[n + 1]))}
             for n in range(nn)]
    return tb, nodes


def pick_ref(table, node, logits):
    """Temperature 0: (token, next node) by the header's steps 1 - 5 with numpy float32 adds."""
    x = np.array(logits, dtype=np.float32)
    if table is None:
        return first_max(x), node
    tb, nodes = parse(table)
    for t, v in tb:
        x[t] = np.float32(x[t] + v)
    if node != DEAD:
        for t, (boost, _) in nodes[node].items():
            x[t] = np.float32(x[t] + boost)
    tok = first_max(x)
    return tok, advance_ref(nodes, node, tok)


def first_max(x):
    """The first maximum; an all -inf or all-NaN row gives 0 (np.argmax would give the first NaN of a mixed row: NaN never wins here)."""
    best, at = -np.inf, None
    for j, v in enumerate(x):
        if v > best or (at is None and v == best):
            best, at = v, j
    return 0 if at is None else at


def advance_ref(nodes, node, tok):
    if tok in (0, 3):
        return 0
    if node == DEAD:
        return DEAD
    return nodes[node][tok][1] if tok in nodes[node] else DEAD


# ---- crafted cases: one bias set and rows that exercise every rule, for any V >= 5 ----
# pieces 1, 2, 4 are always below V; the set is the same for every V so that one engine-side set serves all row lengths
CRAFT_TOKENS = [(1, 0.75), (2, -np.inf), (4, np.float32(1.25 * 2.0 ** -24))]
CRAFT_KEYWORDS = [([1, 2], 4.0), ([1, 4], 1.5), ([4], 0.5), ([1], 1.0), ([1, 2, 4], 2.5), ([4], 0.25)]


# token 4 at the root, from l = 1: (l + v) + k = 1.5 + 2^-23, but l + (v + k) = 1.5
ORDER_RIGHT = np.float32(np.float32(np.float32(1.0) + CRAFT_TOKENS[2][1]) + np.float32(0.5))
ORDER_WRONG = np.float32(np.float32(1.0) + np.float32(CRAFT_TOKENS[2][1] + np.float32(0.5)))


def crafted_set():
    return CRAFT_TOKENS, CRAFT_KEYWORDS


def crafted_rows(V, seed=0):
    """[(row, node)]: rows of V float32 and the node they are picked at.  The set of crafted_set() compiles to
    root -1-> 1, root -4-> 2 (a leaf), 1 -2-> 3, 1 -4-> 4 (a leaf), 3 -4-> 5 (a leaf)."""
    rng = np.random.default_rng(1000 + V + seed)
    base = lambda: (rng.standard_normal(V) * 0.5).astype(np.float32)
    out = []
    r = base(); r[2] = 9.0                       # the raw arg-max is banned: the pick moves elsewhere
    out += [(r, 0), (r, DEAD)]
    r = np.full(V, -1.0, dtype=np.float32); r[1] = 0.25 - 0.75 - 4.0; r[0] = 0.25
    out += [(r, 0)]                              # unbiased: 0 wins.  At the root token 1 gains 0.75 + 4.0 and TIES token 0: the lower id wins
    r = np.full(V, -1.0, dtype=np.float32); r[1] = -0.75 - 4.0 + 0.25; r[V - 1] = 0.25
    out += [(r, 0)]                              # the tie the other way round: token 1 (boosted) against V - 1 (raw): 1 wins
    r = np.full(V, -8.0, dtype=np.float32); r[4] = 1.0
    out += [(r, 0), (r, 1), (r, 3), (r, 2), (r, DEAD)]   # token 4 carries a bias AND a boost at the root, at node 1 and at node 3
    r = r.copy(); r[0] = ORDER_WRONG
    out += [(r, 0), (r, DEAD)]                   # at the root (l + v) + k beats token 0 by one ulp; l + (v + k) would tie and pick 0
    r = np.full(V, -np.inf, dtype=np.float32)
    out += [(r, 0), (r, 5)]                      # everything banned: token 0
    r = np.full(V, np.nan, dtype=np.float32)
    out += [(r, 1)]
    r = base(); r[0] = 7.0
    out += [(r, 1), (r, DEAD)]                   # token 0: back to the root from an inner node and from DEAD
    r = base(); r[3] = 7.0
    out += [(r, 3), (r, DEAD)]                   # token 3 likewise
    r = base(); r[1] = 7.0
    out += [(r, 0), (r, 1), (r, DEAD)]           # a child token at the root; the same token where it is no child; DEAD stays DEAD
    r = base(); r[V - 1] = 7.0
    out += [(r, 0), (r, 4)]                      # a non-child token: DEAD (unless V - 1 is 4: then a child of the root)
    for node in (0, 1, 2, 3, 4, 5, DEAD):        # plain random rows at every node
        out.append((base(), node))
    return out
