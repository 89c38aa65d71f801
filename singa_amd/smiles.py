"""The host side of grammar-constrained sampling (`sample(..., grammar="smiles")`): token classes of a SMILES vocabulary and
the packed per-row state of the rule that include/singa_hip_gen.h states and `singa_sample_token_grammar` evaluates on the
device.  The rule itself is not restated here - only what the host has to prepare: one class byte per vocabulary entry and
the fresh state.

Scope of the rule: syntax only - balanced branches, paired ring-closure digits, no dangling bond symbol, and a '$' before the
columns run out.  Not covered: chemical validity (valence, aromaticity, duplicate ring bonds such as C1C1), %nn closures (the
vocabulary has none), a bond symbol in front of a closing ring digit (never drawn), beam search."""
import numpy as np

NONE, ATOM, BOND, OPEN, CLOSE, RING, DOT, EOS = range(8)        # token classes; prev codes 1-6 are the classes' own
START, BONDX = 7, 8                                             # further prev codes: fresh row, bond symbol after '(' or ')'
FRESH = START                                                   # state word of a fresh row: prev = START, everything else 0
GRAMMARS = ("smiles",)

_ORGANIC = {"B", "C", "N", "O", "P", "S", "F", "I", "Br", "Cl", "b", "c", "n", "o", "p", "s"}
_FIXED = {"(": OPEN, ")": CLOSE, ".": DOT, "$": EOS}


def classify(voc):
    """uint8 [V]: low nibble = class of the token string, high nibble = ring digit index 0..8 ('1' .. '9')."""
    out = np.zeros(len(voc), np.uint8)
    for i, tok in enumerate(voc):
        tok = str(tok)
        if tok in _ORGANIC or (len(tok) > 2 and tok[0] == "[" and tok[-1] == "]"):
            out[i] = ATOM
        elif len(tok) == 1 and tok in "-=#/\\:":
            out[i] = BOND
        elif len(tok) == 1 and tok in "123456789":
            out[i] = RING | (int(tok) - 1) << 4
        else:
            out[i] = _FIXED.get(tok, NONE)
    return out


def pack(prev, depth=0, ring=0, here=0):
    return int(prev) | int(depth) << 4 | int(ring) << 10 | int(here) << 19


def unpack(state):
    """-> (prev, depth, ring, here); works on ints and integer arrays"""
    return state & 15, state >> 4 & 63, state >> 10 & 511, state >> 19 & 511


def check_arguments(grammar, voc, max_length, suppress=()):
    """The argument check of `sample(..., grammar=...)`: raises ValueError for what the rule cannot work with; returns the class
    bytes otherwise (None for grammar=None)."""
    if grammar is None:
        return None
    if grammar not in GRAMMARS:
        raise ValueError(f"sample: unknown grammar {grammar!r} (known: {', '.join(GRAMMARS)})")
    if max_length < 3:
        raise ValueError(f"sample: grammar={grammar!r} needs max_length >= 3 ('&', one atom, '$'), got {max_length}")
    voc = [str(v) for v in voc]
    cls = classify(voc)
    if "$" not in voc or cls[voc.index("$")] != EOS:
        raise ValueError("sample: the grammar ends a row with '$', which the vocabulary does not hold as its end token")
    gone = {str(s) for s in suppress}
    kept = lambda c: [v for v, k in zip(voc, cls & 15) if k == c and v not in gone]
    if not kept(ATOM):
        raise ValueError("sample: suppress removes every atom token; the grammar could draw nothing")
    if not kept(EOS):
        raise ValueError("sample: suppress removes '$'; under the grammar every row has to end")
    if kept(OPEN) and not kept(CLOSE):
        raise ValueError("sample: suppress removes ')' while '(' stays; an opened branch could never be closed")
    return cls
