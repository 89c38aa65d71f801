"""The host side of grammar-constrained sampling (`sample(..., grammar="smiles")`): token classes of a SMILES vocabulary and
the packed per-row state of the rule that include/singa_hip_gen.h states and `singa_sample_token_grammar` evaluates on the
device.  The rule itself is not restated here - only what the host has to prepare: one class byte per vocabulary entry and
the fresh state.

Scope of the "smiles" rule: syntax only - balanced branches, paired ring-closure digits, no dangling bond symbol, and a '$'
before the columns run out.  Not covered: chemical validity (valence, aromaticity, duplicate ring bonds such as C1C1), %nn
closures (the vocabulary has none), a bond symbol in front of a closing ring digit (never drawn).  Beam search takes both
rules through `BeamSearch.beam_search_device` (include/singa_hip_beam.h).

`grammar="valence"` (include/singa_hip_valence.h states the rule, `singa_sample_token_valence` evaluates it) adds a
bonding-capacity rule to the syntax: no atom of a drawn row carries more bond order than the capacity of its token
(`capacity`).  The host prepares one more byte per vocabulary entry for it, and the class bytes of the bond tokens carry
their order (`classify_orders`).  A necessary condition for validity, not a sufficient one: aromaticity, kekulisation and
duplicate ring bonds stay uncovered."""
import functools
import re

import numpy as np

NONE, ATOM, BOND, OPEN, CLOSE, RING, DOT, EOS = range(8)        # token classes; prev codes 1-6 are the classes' own
START, BONDX = 7, 8                                             # further prev codes: fresh row, bond symbol after '(' or ')'
FRESH = START                                                   # state word of a fresh row: prev = START, everything else 0
GRAMMARS = ("smiles", "valence")

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


def classify_orders(voc):
    """`classify` for the valence rule: the high nibble of a BOND token holds its order - 1 (1 for '=', 2 for '#', 0 for every
    other bond symbol), which the SMILES rule does not read."""
    out = classify(voc)
    for i, tok in enumerate(voc):
        if out[i] == BOND:
            out[i] |= {"=": 1, "#": 2}.get(str(tok), 0) << 4
    return out


# Upper bounds of the bond order an element's atom carries, so that no valid string is excluded (include/singa_hip_valence.h)
_CAPACITY = {"B": 3, "C": 4, "Si": 4, "N": 3, "O": 2, "P": 5, "As": 5, "S": 6, "Se": 6, "F": 1, "Cl": 1, "Br": 1, "I": 1}
_CHARGE_ADDS = {"N", "P", "As", "O", "S", "Se", "F", "Cl", "Br", "I"}         # the N, O and halogen groups: + charge
_BRACKET = re.compile(r"\[(\d+)?(se|as|[bcnops]|[A-Z][a-z]?)(@{0,2})(?:H(\d?))?(\+{1,3}|-{1,3}|[+-]\d)?\]")
UNCONSTRAINED = 7


def capacity(voc):
    """uint8 [V]: the bonding capacity 0..7 of every ATOM token, 0 for every other token - the most bond order the valence
    rule lets the token's atom carry.  UPPER bounds, so that no valid string is ever excluded:

        B 3    C, Si 4    N 3    O 2    P, As 5    S, Se 6    F, Cl, Br, I 1

    A lower-case (aromatic) symbol takes its element's value.  A bracket atom is read as
    [isotope? element chirality? H-count? charge?]: its capacity is table[element] + the charge term - the H count, clamped
    to 0..7, with the charge term + charge for the N, O and halogen groups ([N+] 4, [O-] 1, [Cl-] 0), - charge for B ([B-] 4)
    and - |charge| for C and Si.  An element outside the table, or a bracket that does not read this way, gets 7 (no
    constraint)."""
    cls = classify(voc)
    out = np.zeros(len(voc), np.uint8)
    for i, tok in enumerate(voc):
        if cls[i] != ATOM:
            continue
        tok = str(tok)
        if tok[0] != "[":
            out[i] = _CAPACITY[tok.capitalize()]
            continue
        m = _BRACKET.fullmatch(tok)
        element = m.group(2).capitalize() if m else None
        if element not in _CAPACITY:
            out[i] = UNCONSTRAINED
            continue
        hydrogens = 0 if m.group(4) is None else int(m.group(4) or 1)
        sign = m.group(5) or ""
        charge = 0 if not sign else (int(sign[1:]) if sign[1:].isdigit() else len(sign)) * (1 if sign[0] == "+" else -1)
        term = charge if element in _CHARGE_ADDS else -charge if element == "B" else -abs(charge)
        out[i] = min(max(_CAPACITY[element] + term - hydrogens, 0), UNCONSTRAINED)
    return out


ANCHOR = 4              # the valence rule finishes every row with atoms of at least this capacity


def pack(prev, depth=0, ring=0, here=0):
    return int(prev) | int(depth) << 4 | int(ring) << 10 | int(here) << 19


def unpack(state):
    """-> (prev, depth, ring, here); works on ints and integer arrays"""
    return state & 15, state >> 4 & 63, state >> 10 & 511, state >> 19 & 511


def check_arguments(grammar, voc, max_length, suppress=()):
    """The argument check of `sample(..., grammar=...)`: raises ValueError for what the rule cannot work with; returns the class
    bytes otherwise (None for grammar=None; `classify_orders` for "valence", which also needs an atom token of capacity >= 4
    that `suppress` leaves: the rule's shortest completion closes the open rings on such atoms)."""
    if grammar is None:
        return None
    if grammar not in GRAMMARS:
        raise ValueError(f"sample: unknown grammar {grammar!r} (known: {', '.join(GRAMMARS)})")
    if max_length < 3:
        raise ValueError(f"sample: grammar={grammar!r} needs max_length >= 3 ('&', one atom, '$'), got {max_length}")
    voc = [str(v) for v in voc]
    cls = classify_orders(voc) if grammar == "valence" else classify(voc)
    if "$" not in voc or cls[voc.index("$")] != EOS:
        raise ValueError("sample: the grammar ends a row with '$', which the vocabulary does not hold as its end token")
    gone = {str(s) for s in suppress}
    kept = lambda c: [v for v, k in zip(voc, cls & 15) if k == c and v not in gone]
    if not kept(ATOM):
        raise ValueError("sample: suppress removes every atom token; the grammar could draw nothing")
    if grammar == "valence" and not any(c >= ANCHOR and k == ATOM and v not in gone for v, k, c in zip(voc, cls & 15, capacity(voc))):
        raise ValueError(f"sample: grammar='valence' needs an atom token of capacity >= {ANCHOR} that suppress leaves (such as 'C'): "
                         "its open rings could not be closed otherwise")
    if not kept(EOS):
        raise ValueError("sample: suppress removes '$'; under the grammar every row has to end")
    if kept(OPEN) and not kept(CLOSE):
        raise ValueError("sample: suppress removes ')' while '(' stays; an opened branch could never be closed")
    return cls


# ------------------------------------------------------------------------------------------------ forced tokens: the host side
# `sample(..., forced=...)` / `score` (singa_amd/model/Sampling.py; include/singa_hip_force.h states what the kernel does with a
# forced token): spelling text in the vocabulary, laying prefixes out as the matrix the kernel reads, and walking that matrix
# through the library's own rule before anything is launched - the kernel takes a forced token whether or not the rule allows it.
@functools.lru_cache(maxsize=8)
def _spelling(voc):
    """-> (the set of entries, first character -> the entries that start with it, longest first)"""
    by_first = {}
    for v in sorted(set(voc) - {""}, key=len, reverse=True):
        by_first.setdefault(v[0], []).append(v)
    return frozenset(voc), by_first


def tokenize(text, voc):
    """The vocabulary entries that spell `text`, greedily: a bracket atom whole, otherwise the longest entry that matches
    ('Br' / 'Cl' before 'B' / 'C').  ValueError, naming the position, for text the vocabulary cannot spell."""
    known, by_first = _spelling(tuple(str(v) for v in voc))
    out, i = [], 0
    while i < len(text):
        if text[i] == "[":
            j = text.find("]", i)
            if j < 0:
                raise ValueError(f"tokenize: '[' at position {i} of {text!r} is never closed")
            tok = text[i:j + 1]
            if tok not in known:
                raise ValueError(f"tokenize: the vocabulary has no entry {tok!r} (position {i} of {text!r})")
        else:
            tok = next((v for v in by_first.get(text[i], ()) if text.startswith(v, i)), None)
            if tok is None:
                raise ValueError(f"tokenize: no vocabulary entry matches {text[i]!r} at position {i} of {text!r}")
        out.append(tok)
        i += len(tok)
    return out


def encode(items, voc, max_length, end=False):
    """int64 [len(items), max_length], -1 where nothing is forced: column 0 is '&', columns 1..n the tokens of item i, column
    n + 1 '$' if `end`.  An item is a string (`tokenize`) or a sequence of token strings or ids.  ValueError for an item that
    does not fit into the columns."""
    voc = [str(v) for v in voc]
    index = {}
    for i, v in enumerate(voc):
        index.setdefault(v, i)                                         # as list.index: the first of equal entries
    out = np.full((len(items), max_length), -1, np.int64)
    for r, item in enumerate(items):
        toks = tokenize(item, voc) if isinstance(item, str) else list(item)
        ids = []
        for c, t in enumerate(toks):
            if isinstance(t, str):
                if t not in index:
                    raise ValueError(f"encode: item {r}, token {c}: the vocabulary has no entry {t!r}")
                ids.append(index[t])
            else:
                if not 0 <= int(t) < len(voc):
                    raise ValueError(f"encode: item {r}, token {c}: id {int(t)} is outside the vocabulary of {len(voc)}")
                ids.append(int(t))
        n = len(ids) + (1 if end else 0)
        if n > max_length - 1:
            raise ValueError(f"encode: item {r} takes {len(ids)} tokens{' and its $' if end else ''}; max_length = {max_length} "
                             f"has {max_length - 1} columns after '&'")
        out[r, 0] = index["&"]
        out[r, 1:1 + len(ids)] = ids
        if end:
            out[r, 1 + len(ids)] = index["$"]
    return out


def check_forced(forced, voc, max_length, grammar=None):
    """The argument check of `sample(..., forced=...)`, on the CPU: `forced` [rows, max_length] integers, a value outside the
    vocabulary (-1) = a free column.  Column 0 must be '&' or free, a row's forced columns must be one run that starts at column
    1 (no free column in front of a forced one), and nothing may be forced behind a forced '$'.  Under `grammar` every forced
    token is walked through the library's rule of that grammar (`singa_smiles_rule_host` / `singa_valence_rule_host`: the
    functions the kernel evaluates), from the fresh
    state with rem = max_length - 2 - t at step t, so a prefix that leaves too few columns to finish is refused as well.  One
    exception: a row forced to '$' in column 1 is an empty row (what `score` pads ragged lists with) and passes under any
    grammar.  ValueError names row, column and token of the first refusal; returns the matrix as a contiguous int64 array."""
    voc = [str(v) for v in voc]
    V = len(voc)
    f = np.ascontiguousarray(np.asarray(forced))
    if f.ndim != 2 or f.shape[1] != max_length or f.dtype.kind not in "iu":
        raise ValueError(f"forced: an integer matrix [rows, max_length = {max_length}] is expected, got {f.dtype} {f.shape}")
    f = f.astype(np.int64)
    cls = check_arguments(grammar, voc, max_length)
    is_f = (f >= 0) & (f < V)
    name = lambda r, c: f"row {r}, column {c}, token {voc[f[r, c]]!r}"
    bad0 = np.flatnonzero(is_f[:, 0] & (f[:, 0] != (voc.index("&") if "&" in voc else -1)))
    if len(bad0):
        raise ValueError(f"forced: {name(int(bad0[0]), 0)}: column 0 is the start token '&' (or free)")
    n = np.where(is_f[:, 1:].all(1), max_length - 1, np.argmin(is_f[:, 1:], 1))          # length of the run from column 1
    eos = voc.index("$") if "$" in voc else -1
    for r in np.flatnonzero(is_f[:, 1:].sum(1) != n):
        c = 1 + int(n[r]) + int(np.argmax(is_f[r, 1 + n[r]:]))
        raise ValueError(f"forced: {name(int(r), c)} follows the free column {int(n[r]) + 1}: the forced columns of a row are one "
                         f"run from column 1")
    ended = np.zeros(len(f), bool)
    state = np.full(len(f), FRESH, np.int32)
    vstate = np.zeros((len(f), 2), np.int32)
    filler = (n >= 1) & (f[:, 1] == eos)
    rule = None
    if grammar is not None:
        import ctypes

        from . import _capi, _lib
        rule = _lib.lib().singa_valence_rule_host if grammar == "valence" else _lib.lib().singa_smiles_rule_host
        cap = capacity(voc) if grammar == "valence" else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for t in range(int(n.max()) if len(n) else 0):
        on = np.flatnonzero(n > t)
        tok = f[on, t + 1]
        late = on[ended[on]]
        if len(late):
            r = int(late[0])
            raise ValueError(f"forced: {name(r, t + 1)} stands behind the row's '$'")
        if rule is not None:
            c = np.ascontiguousarray(cls[tok])
            st = np.ascontiguousarray(state[on])
            rem = np.full(len(on), max_length - 2 - t, np.int32)
            ok, nxt = np.zeros(len(on), np.uint8), np.zeros(len(on), np.int32)
            if grammar == "valence":
                k, vs, vnxt = np.ascontiguousarray(cap[tok]), np.ascontiguousarray(vstate[on]), np.zeros((len(on), 2), np.int32)
                _capi.check(_lib.lib(), rule(vp(c), vp(k), vp(st), vp(vs), vp(rem), len(on), vp(ok), vp(nxt), vp(vnxt)),
                            "singa_valence_rule_host")
                vstate[on] = vnxt
            else:
                _capi.check(_lib.lib(), rule(vp(c), vp(st), vp(rem), len(on), vp(ok), vp(nxt)), "singa_smiles_rule_host")
            refused = on[(ok == 0) & ~filler[on]]
            if len(refused):
                r = int(refused[0])
                raise ValueError(f"forced: {name(r, t + 1)}: the {grammar} rule does not let it follow "
                                 f"{''.join(voc[i] for i in f[r, 1:t + 1])!r} with {max_length - 2 - t} columns left after it")
            state[on] = nxt
        ended[on] |= tok == eos
    return f


def check_prefix(forced, voc, batch_size, max_length, grammar=None):
    """`check_forced` for the modes whose rows exchange prefixes (`sample_distinct(..., forced=...)`,
    `beam_search_device(..., forced=...)`; include/singa_hip_prefix.h): `forced` is [batch_size, max_length], ONE prefix per
    pocket.  On top of what `check_forced` demands - one run of forced columns from column 1, and under `grammar` a prefix the
    rule accepts and can still finish - a prefix holds no '$' (a finished string leaves nothing to search for) and leaves at
    least one free column.  ValueError names pocket, column and token of the first refusal; returns the contiguous int64 matrix."""
    voc = [str(v) for v in voc]
    f = np.asarray(forced)
    if f.ndim != 2 or f.shape != (batch_size, max_length) or f.dtype.kind not in "iu":
        raise ValueError(f"forced: one prefix per pocket, an integer matrix [batch_size = {batch_size}, max_length = {max_length}], "
                         f"is expected, got {f.dtype} {f.shape}")
    try:
        f = check_forced(f, voc, max_length, None)
    except ValueError as e:
        raise ValueError(str(e).replace("forced: row", "forced: pocket", 1)) from None
    is_f = (f >= 0) & (f < len(voc))
    name = lambda p, c: f"pocket {p}, column {c}, token {voc[f[p, c]]!r}"
    if "$" in voc:
        for p, c in zip(*np.nonzero(is_f[:, 1:] & (f[:, 1:] == voc.index("$")))):
            raise ValueError(f"forced: {name(int(p), int(c) + 1)}: a prefix holds no '$' - a whole molecule is scored (`score`), not "
                             f"searched")
    full = np.flatnonzero(is_f[:, 1:].all(1))
    if len(full):
        raise ValueError(f"forced: {name(int(full[0]), max_length - 1)}: the prefix leaves no free column of max_length = {max_length}")
    if grammar is not None:
        try:
            check_forced(f, voc, max_length, grammar)
        except ValueError as e:
            raise ValueError(str(e).replace("forced: row", "forced: pocket", 1)) from None
    return f
