"""Helper (no tests): the valence rule of `singa_sample_token_valence` restated in numpy from the text of
include/singa_hip_valence.h - the SMILES rule of tests/grammar_rule.py plus the bonding-capacity rule - and a checker written
separately from it: it builds the molecular graph that a token list spells and sums the bond orders at every atom, without
any of the rule's state.  Shared by tests/test_valence_cpu.py and tests/test_valence_gpu.py."""
import numpy as np

from tests import grammar_rule as G

NONE, ATOM, BOND, OPEN, CLOSE, RING, DOT, EOS, START, BONDX = (G.NONE, G.ATOM, G.BOND, G.OPEN, G.CLOSE, G.RING, G.DOT, G.EOS,
                                                                 G.START, G.BONDX)
FRESH = G.FRESH
MAX_DEPTH = 10


# ------------------------------------------------------------------------------------------------ the rule, restated
def class_bytes(voc):
    """uint8 [V]: the class bytes of grammar_rule's classes, a BOND token carrying its order - 1 in the high nibble"""
    out = np.zeros(len(voc), np.uint8)
    for i, tok in enumerate(voc):
        tok = str(tok)
        if G._Parser.is_atom(tok):
            out[i] = ATOM
        elif G._Parser.is_bond(tok):
            out[i] = BOND | ({"=": 2, "#": 3}.get(tok, 1) - 1) << 4
        elif G._Parser.is_digit(tok):
            out[i] = RING | (int(tok) - 1) << 4
        else:
            out[i] = {"(": OPEN, ")": CLOSE, ".": DOT, "$": EOS}.get(tok, NONE)
    return out


def vpack(att=0, pend=0, first=0, rord=0, stack=()):
    """-> (word 0, word 1): att bits 0-2, pend bits 3-4, first bit 5, rord bits 6-14; stack entry of level l at bits 3l"""
    return att | pend << 3 | first << 5 | rord << 6, sum(int(e) << 3 * l for l, e in enumerate(stack))


def vfields(v0):
    return v0 & 7, v0 >> 3 & 3, v0 >> 5 & 1, v0 >> 6 & 511


def _arrays(*xs):
    return [np.array(a, np.int64) for a in np.broadcast_arrays(*[np.asarray(x, np.int64) for x in xs])]


def _read(st, v0, v1):
    """The fields of a state; a START row reads both valence words as 0.  The stack comes as [..., 10]."""
    prev, depth, ring, here = G.fields(st)
    fresh = prev == START
    v0, v1 = np.where(fresh, 0, v0), np.where(fresh, 0, v1)
    att, pend, first, rord = vfields(v0)
    stack = np.stack([v1 >> 3 * l & 7 for l in range(MAX_DEPTH)], -1)
    return prev, depth, ring, here, att, pend, first, rord, stack


def _write(prev, depth, ring, here, att, pend, first, rord, stack):
    v1 = sum((stack[..., l] & 7) << 3 * l for l in range(MAX_DEPTH))
    return G.pack(prev, depth, ring, here), (att & 7) | pend << 3 | first << 5 | rord << 6, v1


def _order(cl, c, prev, ring, pend, rord, bit):
    """bond order that a token of class `cl` puts on the attach atom (0: none)"""
    link = np.where(pend > 0, pend, 1)
    atom = np.where(np.isin(prev, (START, DOT)), 0, link)
    digit = np.where((ring & bit) == 0, link, np.where((rord & bit) != 0, 2, 1))
    return np.select([cl == ATOM, cl == BOND, cl == RING], [atom, np.minimum((c >> 4) + 1, 3), digit], 0)


def transition(st, v0, v1, c, cap):
    """state after a token of class byte `c` and capacity `cap`; '$' and NONE leave all three words as they are"""
    st, v0, v1, c, cap = _arrays(st, v0, v1, c, cap)
    prev, depth, ring, here, att, pend, first, rord, stack = _read(st, v0, v1)
    cl, bit = c & 15, 1 << np.minimum(c >> 4, 8)
    o = _order(cl, c, prev, ring, pend, rord, bit)
    level = np.arange(MAX_DEPTH)
    top, new = level == (depth - 1)[..., None], level == depth[..., None]
    opening = (cl == RING) & ((ring & bit) == 0)
    is_atom, is_open, is_close = (cl == ATOM)[..., None], (cl == OPEN)[..., None], (cl == CLOSE)[..., None]
    popped = (stack * top).sum(-1)
    n_stack = np.where(is_atom & (first == 1)[..., None] & top, stack - o[..., None], stack)
    n_stack = np.where(is_open & new, att[..., None], n_stack)
    n_stack = np.where(is_close & top, 0, n_stack)
    n_att = np.select([cl == ATOM, cl == CLOSE, cl == RING, cl == DOT], [cap - o, popped, att - o, 0], att)
    n_pend = np.select([cl == ATOM, cl == BOND, opening], [0, o, 0], pend)
    n_first = np.select([cl == ATOM, cl == OPEN], [0, 1], first)
    n_rord = np.where(opening, (rord & ~bit) | np.where(o == 2, bit, 0), rord)
    g_prev, g_depth, g_ring, g_here = G.fields(G.transition(st, c))
    n_st, n_v0, n_v1 = _write(g_prev, g_depth, g_ring, g_here, np.clip(n_att, 0, 7), n_pend, n_first, n_rord, np.clip(n_stack, 0, 7))
    stays = (cl == NONE) | (cl >= EOS)
    return np.where(stays, st, n_st), np.where(stays, v0, n_v0), np.where(stays, v1, n_v1)


def reach(st, v0, v1):
    """E: the largest capacity among the live stack entries and, after an atom, a ring digit or ')', the attach atom"""
    prev, depth, ring, here, att, pend, first, rord, stack = _read(*_arrays(st, v0, v1))
    live = np.arange(MAX_DEPTH) < depth[..., None]
    e = (stack * live).max(-1)
    return np.where(np.isin(prev, (ATOM, RING, CLOSE)), np.maximum(e, att), e)


def need(st, v0, v1):
    """columns of the shortest completion: depth + 1 + a + 2 k - b"""
    st, v0, v1 = _arrays(st, v0, v1)
    prev, depth, ring, here, att, pend, first, rord, stack = _read(st, v0, v1)
    k = G.popcount9(ring)
    a = np.isin(prev, (START, DOT, BOND, BONDX, OPEN))
    e_stack = (stack * (np.arange(MAX_DEPTH) < depth[..., None])).max(-1)
    some = np.zeros(st.shape, bool)
    for d in range(9):                                 # may digit d follow as a CLOSING digit (the budget aside)
        bit = 1 << d
        o = np.where((rord & bit) != 0, 2, 1)
        e_after = np.maximum(e_stack, att - o)         # after a digit the attach atom counts
        some |= ((ring & bit) != 0) & ((here & bit) == 0) & (att >= o) & (((ring & ~bit) == 0) | (e_after >= 1))
    b = (k > 0) & np.isin(prev, (ATOM, RING)) & some
    return depth + 1 + a + 2 * k - b


def allows(st, v0, v1, c, cap, rem, with_need=False):
    """bool (array): may a token of class byte `c` and capacity `cap` follow the state with `rem` columns left after it;
    `with_need`: -> (that, `need` of the state after the token)"""
    st, v0, v1, c, cap, rem = _arrays(st, v0, v1, c, cap, rem)
    prev, depth, ring, here, att, pend, first, rord, stack = _read(st, v0, v1)
    cl, d = c & 15, c >> 4
    bit = 1 << np.minimum(d, 8)
    atomish = np.isin(prev, (ATOM, RING))
    A = atomish | (prev == CLOSE)
    is_open = (ring & bit) != 0
    syntax = np.select(
        [cl == ATOM, cl == BOND, cl == OPEN, cl == CLOSE, cl == DOT, cl == RING, cl == EOS],
        [np.ones_like(A), A | (prev == OPEN), A & (depth < MAX_DEPTH), A & (depth > 0), A,
         (d < 9) & np.where(is_open, atomish & ((here & bit) == 0), atomish | (prev == BOND)), A & (depth == 0) & (ring == 0)],
        False)
    o = _order(cl, c, prev, ring, pend, rord, bit)
    after = transition(st, v0, v1, c, cap)
    ring_after = G.fields(after[0])[2]
    e_after = reach(*after)
    live = np.arange(MAX_DEPTH) < depth[..., None]
    atom_ok = ((o == 0) | ((att >= o) & (cap >= o))) & ((ring == 0) | (e_after >= 1))
    close_ok = (ring == 0) | ((stack * live).max(-1) >= 1)
    digit_ok = np.where(is_open, (att >= o) & ((ring_after == 0) | (e_after >= 1)), (o <= 2) & (att >= o) & (e_after >= 1))
    valence = np.select([cl == ATOM, cl == BOND, cl == OPEN, cl == CLOSE, cl == RING], [atom_ok, att >= o, att >= 1, close_ok, digit_ok],
                        True)
    need_after = need(*after)
    ok = syntax & valence & ((cl == EOS) | (rem >= need_after))
    return (ok, need_after) if with_need else ok


def step(st, v0, v1, c, cap, rem):
    """-> (ok, next state word, next valence words): the state after the token where it is allowed, the given words elsewhere"""
    st, v0, v1, c, cap, rem = _arrays(st, v0, v1, c, cap, rem)
    ok = allows(st, v0, v1, c, cap, rem)
    n = transition(st, v0, v1, c, cap)
    return ok, np.where(ok, n[0], st), np.where(ok, n[1], v0), np.where(ok, n[2], v1)


def replay(tokens, cls, cap, eos):
    """tokens [R, T], every row starting with '&'.  -> (states [R, T - 1, 3]: the three words in front of step t, live [R, T - 1]
    bool: step t was decided, i.e. no '$' in front of it); step t has rem = T - 2 - t."""
    tokens = np.asarray(tokens)
    R, T = tokens.shape
    states, live = np.zeros((R, T - 1, 3), np.int64), np.zeros((R, T - 1), bool)
    s, on = [np.full(R, FRESH, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)], np.ones(R, bool)
    for t in range(T - 1):
        states[:, t], live[:, t] = np.stack(s, -1), on
        tok = np.clip(tokens[:, t + 1], 0, len(cls) - 1)
        on = on & (tokens[:, t + 1] != eos)
        n = transition(*s, np.asarray(cls)[tok], np.asarray(cap)[tok])
        s = [np.where(on, a, b) for a, b in zip(n, s)]
    return states, live


def walks(T, rows, seed, cls, cap, eos, rule="valence", bias=12.0, keep_states=False, weights=None):
    """Random walks under the rule, all rows at once, biased towards '(', digits, bonds, ')' and '.'.  -> dict: tokens [rows, T]
    (column 0 and everything behind a '$' are -1), fewest (the smallest number of allowed tokens at a live step), stuck (live
    steps at which '$' was not allowed and no allowed token had a lower `need`), states (the (state, v0, v1, rem) of every
    live step, if asked for).  rule="smiles": the walk follows grammar_rule alone.  `weights`: {class: weight} in place of the bias."""
    rs = np.random.RandomState(seed)
    V = len(cls)
    cls, cap = np.asarray(cls, np.int64), np.asarray(cap, np.int64)
    w = np.ones(V)
    w[np.isin(cls & 15, (BOND, OPEN, CLOSE, RING, DOT))] = bias
    w[(cls & 15) == EOS] = 3.0
    for k, x in (weights or {}).items():
        w[(cls & 15) == k] = x
    out = np.full((rows, T), -1, np.int64)
    s = [np.full(rows, FRESH, np.int64), np.zeros(rows, np.int64), np.zeros(rows, np.int64)]
    on = np.ones(rows, bool)
    fewest, stuck, seen = V, 0, []
    for t in range(T - 1):
        rem = T - 2 - t
        if rule == "valence":
            m, nd = allows(s[0][:, None], s[1][:, None], s[2][:, None], cls[None], cap[None], rem, with_need=True)
            lower = (m & (nd < need(*s)[:, None])).any(1)
            stuck += int((on & ~m[:, eos] & ~lower).sum())
        else:
            m = G.allows(s[0][:, None], cls[None], rem)
        if keep_states:
            seen.append(np.stack([a[on] for a in s] + [np.full(int(on.sum()), rem)], -1))
        if on.any():
            fewest = min(fewest, int(m[on].sum(1).min()))
        p = np.where(m, w[None], 0.0)
        p[~p.any(1)] = 1.0                                              # (a dead end: counted in `fewest`, the row goes on anywhere)
        cdf = np.cumsum(p, 1)
        tok = (cdf > (rs.rand(rows) * cdf[:, -1])[:, None]).argmax(1)
        out[on, t + 1] = tok[on]
        n = transition(*s, cls[tok], cap[tok])
        on = on & (tok != eos)
        s = [np.where(on, a, b) for a, b in zip(n, s)]
    return {"tokens": out, "fewest": fewest, "stuck": stuck, "states": np.concatenate(seen) if keep_states else None}


# ------------------------------------------------------------------------------------------------ the checker
def bond_sums(toks):
    """The molecular graph of a syntactically complete token list: -> [(atom token, sum of the orders of its bonds)], one entry
    per atom in the order written.  A bond symbol counts 2 for '=', 3 for '#', 1 otherwise; atoms that follow each other
    without a symbol are joined by a single bond, '.' joins nothing; a ring bond has the order written at either digit."""
    value = {"=": 2, "#": 3}
    atoms, sums = [], []
    last, symbol, joined = None, None, True         # the atom a bond would start from; the bond symbol waiting; '.' not seen
    branch, rings = [], {}
    for t in toks:
        if G._Parser.is_atom(t):
            atoms.append(t), sums.append(0)
            if last is not None and joined:
                o = value.get(symbol, 1)
                sums[last] += o
                sums[-1] += o
            last, symbol, joined = len(atoms) - 1, None, True
        elif G._Parser.is_bond(t):
            symbol = t
        elif G._Parser.is_digit(t):
            if t in rings:
                other, sym = rings.pop(t)
                o = max(value.get(symbol, 1), value.get(sym, 1))
                sums[last] += o
                sums[other] += o
            else:
                rings[t] = (last, symbol)
            symbol = None
        elif t == "(":
            branch.append(last)
        elif t == ")":
            last, joined = branch.pop(), True
        elif t == ".":
            joined = False
        else:
            raise ValueError(f"bond_sums: token {t!r}")
    if rings or branch:
        raise ValueError(f"bond_sums: unclosed ring or branch in {''.join(toks)!r}")
    return list(zip(atoms, sums))


def over_capacity(toks, capacity):
    """[(index of the atom, token, bonds, capacity)] for every atom of `toks` with more bond order than `capacity[token]`"""
    return [(i, a, n, capacity[a]) for i, (a, n) in enumerate(bond_sums(toks)) if n > capacity[a]]


def texts_of(tokens, voc, eos):
    """token strings of every row of `walks` output between column 0 and '$'; None for a row without '$'"""
    out = []
    for row in tokens:
        row = [int(x) for x in row[1:]]
        out.append([voc[x] for x in row[:row.index(eos)]] if eos in row else None)
    return out


# ------------------------------------------------------------------------------------------------ vocabularies
def wide_vocabulary():
    """200 distinct entries: the shipped vocabulary and further bracket atoms (isotopes, H counts, charges), shuffled, so that
    structure tokens sit in every register group of a lane and capacities 0..7 all occur"""
    from tests.helpers import smi_voc
    base = list(dict.fromkeys(smi_voc()))
    extra = [f"[{iso}{el}{h}{ch}]" for el in ("C", "N", "O", "S", "P", "B", "Si", "Cl", "Se", "As") for iso in ("", "13")
             for h in ("", "H", "H2") for ch in ("", "+", "-")]
    voc = base + [e for e in extra if e not in base][:200 - len(base)]
    assert len(voc) == 200
    return [voc[i] for i in np.random.RandomState(200).permutation(200)]
