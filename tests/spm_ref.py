"""Test-side restatement of SentencePiece's DecodeIds from the piece table recorded in tests/golden/spm/vectors.json, so that
GPU tests need no Python `sentencepiece`.  It covers what the golden models are: dummy prefix and remove_extra_whitespaces on,
the default unk surface.  tests/test_spm_cpu.py pins it to the module itself."""
import functools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spm")
WS, UNK_SURFACE, REPLACEMENT = "\u2581".encode(), " \u2047 ".encode(), "\ufffd".encode()


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "vectors.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def table(model):
    """[(piece bytes, type name)] of a golden model."""
    return [(bytes.fromhex(p), t) for p, t in vectors()["models"][model]["pieces"]]


def _flush(run):
    """A run of byte pieces as UTF-8: U+FFFD for every byte that starts no well-formed character."""
    def well_formed(chunk):
        try:
            return bool(chunk.decode("utf-8"))  # strict: no overlong forms, no surrogates, nothing beyond U+10FFFF
        except UnicodeDecodeError:
            return False
    out, i = b"", 0
    while i < len(run):
        b = run[i]
        k = 1 if b < 0x80 else 2 if 0xc0 <= b < 0xe0 else 3 if 0xe0 <= b < 0xf0 else 4 if 0xf0 <= b < 0xf8 else 0
        chunk = run[i:i + k]
        if k and len(chunk) == k and well_formed(chunk):
            out, i = out + chunk, i + k
        else:
            out, i = out + REPLACEMENT, i + 1
    return out


def decode(model, ids):
    """DecodeIds -> bytes.  An id outside the table raises IndexError."""
    pieces, out, run = table(model), b"", b""
    for i in ids:
        if not 0 <= i < len(pieces):
            raise IndexError(f"piece id {i} is out of range")
        piece, kind = pieces[i]
        if kind == "BYTE":
            run += bytes([int(piece[3:5], 16)])
            continue
        out, run = out + _flush(run), b""
        if kind == "UNKNOWN":
            out += UNK_SURFACE
        elif kind != "CONTROL":
            if not out and piece.startswith(WS):  # nothing decoded yet: the dummy prefix goes
                piece = piece[len(WS):]
            out += piece.replace(WS, b" ")
    return out + _flush(run)
