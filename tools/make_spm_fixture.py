#!/usr/bin/env python3
"""Developer tool (never run by a test): trains the small SentencePiece models under tests/golden/spm/ with the Python
`sentencepiece` module on this repository's own prose and records what the module itself encodes and
decodes into vectors.json.  The native tokenizer (csrc/dsm_spm.h) is held to these bytes.

    python tools/make_spm_fixture.py

Training is deterministic for a given corpus, but the corpus is the current text of the two documents: a run after they have
changed writes different (equally valid) models and vectors.  Commit the models and vectors.json together.

Byte strings (pieces, texts) are stored as hex in vectors.json: some texts are malformed UTF-8 on purpose, and the
stand-alone sanitizer program reads the file without a JSON library.
"""
import io
import json
import os
import random
import re

import sentencepiece as spm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "spm")
TYPE_NAMES = {1: "NORMAL", 2: "UNKNOWN", 3: "CONTROL", 4: "USER_DEFINED", 5: "UNUSED", 6: "BYTE"}


def prose():
    text = ""
    for name in ("DESIGN.md", "SURVEY.md"):
        with open(os.path.join(ROOT, name), encoding="utf-8") as f:
            text += f.read() + "\n"
    return text


def train(sentences, **kw):
    buf = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(sentences), model_writer=buf, pad_id=3, unk_id=0, bos_id=1, eos_id=2,
                                   minloglevel=2, num_threads=1, **kw)
    return buf.getvalue()


def piece_table(sp):
    out = []
    for i in range(sp.get_piece_size()):
        t = 2 if sp.is_unknown(i) else 3 if sp.is_control(i) else 6 if sp.is_byte(i) else 5 if sp.is_unused(i) else 1
        out.append([sp.id_to_piece(i).encode("utf-8").hex(), TYPE_NAMES[t]])
    return out


FIXED_TEXTS = [
    b"", b" ", b"   ", b"hello", b"hello world",
    b"the", b"engine", b"decodes", b"frames", b"now",  # single words: the TTS text path encodes word by word
    b"  hello   world  ", b"the engine decodes frames", b"a", b"zzzz",
    "café naïve à la carte".encode(), "Ｈｅｌｌｏ １２３".encode(),  # full-width
    "ﬁne ① ½ ™ Å".encode(), "é å".encode(),  # ligature, circled digit, fraction; combining marks
    "日本語 中文".encode(), "\U0001f600 ok \U0001f680".encode(), "▁ ▁▁x▁".encode(),
    "tab\there\nnewline\r\n".encode(), " nbsp　ideographic em".encode(), b"<unk> <s> </s> <pad> <0x41>",
    b"\xff", b"ab\x80cd", b"\xc3", b"\xe2\x96", b"x\xf0\x9f\x98y", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80", b"ok \xfe\xff end",
    "� literal".encode(), b"UPPER lower MiXeD 0123456789", b"a.b,c;d:e!f?g", b"word " * 20,
]


def make_texts(sp, rng, n):
    texts = list(FIXED_TEXTS)
    pieces = [sp.id_to_piece(i) for i in range(sp.get_piece_size())]
    alphabet = "abcdefghijklmnopqrstuvwxyz"
    while len(texts) < n:
        kind = rng.randrange(4)
        if kind == 0:  # words made of the model's own pieces
            s = "".join(rng.choice(pieces).replace("▁", " ") for _ in range(rng.randrange(1, 9))).encode()
        elif kind == 1:  # lower-case words with ragged spacing
            s = "".join(rng.choice(alphabet + "   ") for _ in range(rng.randrange(1, 40))).encode()
        elif kind == 2:  # scalars from several blocks, some outside every vocabulary
            s = "".join(chr(rng.choice([rng.randrange(0x20, 0x7f), rng.randrange(0xa0, 0x250), rng.randrange(0xff01, 0xff5f),
                                        rng.randrange(0x4e00, 0x4f00), rng.randrange(0x1f600, 0x1f640), 0x20]))
                        for _ in range(rng.randrange(1, 16))).encode()
        else:  # a valid string with bytes knocked out or thrown in
            b = bytearray("".join(rng.choice(alphabet + " é中") for _ in range(rng.randrange(1, 12))).encode())
            for _ in range(rng.randrange(1, 4)):
                b.insert(rng.randrange(len(b) + 1), rng.randrange(0x80, 0x100))
            s = bytes(b)
        texts.append(s)
    return texts


def make_id_runs(sp, rng, n):
    V = sp.get_piece_size()
    byte_ids = [i for i in range(V) if sp.is_byte(i)]
    runs = [[], [0], [1], [2], [3], [0, 0], [1, 2, 3], [0, 3], [3, 0]]  # control ids, unk, the STT word terminators 0 and 3
    normal = [i for i in range(V) if not (sp.is_byte(i) or sp.is_control(i) or sp.is_unknown(i))]
    runs += [[normal[0]], [normal[-1], 0, normal[0]], [1, normal[3], 2], [normal[5], 3], [0, normal[5]]]
    if byte_ids:
        b = {int(sp.id_to_piece(i)[3:5], 16): i for i in byte_ids}
        runs += [[b[0xc3], b[0xa9]], [b[0xc3]], [b[0xa9]], [b[0xc3], normal[0], b[0xa9]], [b[0xe4], b[0xb8], b[0xad]],
                 [b[0xe4], b[0xb8]], [b[0xf0], b[0x9f], b[0x98], b[0x80]], [b[0x41], normal[1]], [b[0xff], b[0x41]],
                 [normal[2], b[0xe2], b[0x96], b[0x81], normal[2]], [b[0x20], normal[0]], [1, b[0x41], normal[0]]]
    while len(runs) < n:
        k = rng.randrange(1, 10)
        pool = normal if rng.random() < 0.6 else list(range(V))
        run = [rng.choice(pool) for _ in range(k)]
        if byte_ids and rng.random() < 0.3:
            at = rng.randrange(len(run) + 1)
            run[at:at] = [rng.choice(byte_ids) for _ in range(rng.randrange(1, 5))]
        runs.append(run)
    return runs


def main():
    os.makedirs(OUT, exist_ok=True)
    text = prose()
    lines = [l.strip() for l in text.splitlines() if l.strip()]
    lower = [" ".join(re.findall(r"[a-z]+", l.lower())) for l in lines]
    lower = [l for l in lower if l]
    models = {
        "uni512_nfkc_bf": train(lines, model_type="unigram", vocab_size=512, normalization_rule_name="nmt_nfkc", byte_fallback=True,
                                character_coverage=0.995),
        "uni64": train(lower, model_type="unigram", vocab_size=64, normalization_rule_name="identity"),
        "uni40": train(lower, model_type="unigram", vocab_size=40, normalization_rule_name="identity"),
    }
    refused = {"bpe64": train(lower, model_type="bpe", vocab_size=64, normalization_rule_name="identity")}
    vectors = {"models": {}, "refused": [name + ".model" for name in refused]}
    for name, blob in list(models.items()) + list(refused.items()):
        with open(os.path.join(OUT, name + ".model"), "wb") as f:
            f.write(blob)
    for name, blob in models.items():
        sp = spm.SentencePieceProcessor(model_proto=blob)
        rng = random.Random("dsm-spm-" + name)
        enc = [[t.hex(), sp.encode(t)] for t in make_texts(sp, rng, 200)]
        dec = [[ids, sp.decode(ids).encode("utf-8").hex()] for ids in make_id_runs(sp, rng, 200)]
        vectors["models"][name] = {
            "file": name + ".model", "special_ids": [sp.unk_id(), sp.bos_id(), sp.eos_id(), sp.pad_id()],
            "pieces": piece_table(sp), "encode": enc, "decode": dec}
        print(f"{name}: {len(blob)} bytes, {sp.get_piece_size()} pieces, {len(enc)} texts, {len(dec)} id runs")
    with open(os.path.join(OUT, "vectors.json"), "w") as f:
        json.dump(vectors, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
