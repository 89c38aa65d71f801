"""Helper (no tests): the SMILES rule of `singa_sample_token_grammar` restated in numpy from the text of
include/singa_hip_gen.h, and an acceptor written separately from it - a recursive-descent parser over token strings - which
decides whether what the rule produced is a syntactically complete SMILES string.  Shared by tests/test_grammar_cpu.py and
tests/test_grammar_gpu.py."""
import numpy as np

# ------------------------------------------------------------------------------------------------ the rule, restated
NONE, ATOM, BOND, OPEN, CLOSE, RING, DOT, EOS = range(8)
START, BONDX = 7, 8
FRESH = START


def pack(prev, depth=0, ring=0, here=0):
    return prev | depth << 4 | ring << 10 | here << 19


def fields(st):
    return st & 15, st >> 4 & 63, st >> 10 & 511, st >> 19 & 511


def popcount9(x):
    return sum((x >> b & 1) for b in range(9))


def transition(st, c):
    """state after a token of class byte `c` (ints or int arrays); '$' and NONE leave it as it is"""
    st, c = np.asarray(st, np.int64), np.asarray(c, np.int64)
    cl, bit = c & 15, 1 << np.minimum(c >> 4, 8)
    prev, depth, ring, here = fields(st)
    opening = (cl == RING) & ((ring & bit) == 0)
    new_here = np.where(cl == ATOM, 0, np.where(opening, here | bit, here))
    new_ring = np.where(cl == RING, ring ^ bit, ring)
    new_depth = depth + (cl == OPEN) - (cl == CLOSE)
    new_prev = np.where((cl == BOND) & ~np.isin(prev, (ATOM, RING)), BONDX, cl)
    out = pack(new_prev, new_depth, new_ring, new_here)
    return np.where((cl == NONE) | (cl >= EOS), st, out)


def need(st):
    prev, depth, ring, here = fields(np.asarray(st, np.int64))
    a = np.isin(prev, (START, DOT, BOND, BONDX, OPEN)) | ((ring != 0) & ((prev == CLOSE) | ((ring & here) != 0)))
    return a + popcount9(ring) + depth + 1


def allows(st, c, rem):
    """bool (array): may a token of class byte `c` follow state `st` with `rem` columns left after it"""
    st, c, rem = np.asarray(st, np.int64), np.asarray(c, np.int64), np.asarray(rem, np.int64)
    cl, d = c & 15, c >> 4
    bit = 1 << np.minimum(d, 8)
    prev, depth, ring, here = fields(st)
    atomish = np.isin(prev, (ATOM, RING))
    A = atomish | (prev == CLOSE)
    is_open = (ring & bit) != 0
    gram = np.select(
        [cl == ATOM, cl == BOND, cl == OPEN, cl == CLOSE, cl == DOT, cl == RING, cl == EOS],
        [np.ones_like(A), A | (prev == OPEN), A & (depth < 63), A & (depth > 0), A,
         (d < 9) & np.where(is_open, atomish & ((here & bit) == 0), atomish | (prev == BOND)), A & (depth == 0) & (ring == 0)],
        False)
    budget = (cl == EOS) | (rem >= need(transition(st, c)))
    return gram & budget


def step(st, c, rem):
    """-> (ok, next_state): next_state is the state after the token where it is allowed, `st` elsewhere"""
    ok = allows(st, c, rem)
    return ok, np.where(ok, transition(st, c), st)


def mask(st, cls, rem):
    """bool [V]: the tokens of the vocabulary with class bytes `cls` that may follow the one state `st`"""
    return allows(np.full(len(cls), st), cls, np.full(len(cls), rem))


def replay(tokens, cls, eos):
    """tokens [R, T], every row starting with '&'.  -> (states [R, T - 1]: the state in front of step t, live [R, T - 1] bool:
    step t was decided, i.e. no '$' in front of it); step t has rem = T - 2 - t."""
    tokens = np.asarray(tokens)
    R, T = tokens.shape
    states, live = np.zeros((R, T - 1), np.int64), np.zeros((R, T - 1), bool)
    st, on = np.full(R, FRESH, np.int64), np.ones(R, bool)
    for t in range(T - 1):
        states[:, t], live[:, t] = st, on
        tok = tokens[:, t + 1]
        on = on & (tok != eos)
        st = np.where(on, transition(st, np.asarray(cls)[np.clip(tok, 0, len(cls) - 1)]), st)
    return states, live


# ------------------------------------------------------------------------------------------------ the acceptor
#   smiles        := chain END
#   chain         := branched_atom ( (bond | '.')? branched_atom )*
#   branched_atom := atom ( bond? DIGIT )* ( '(' bond? chain ')' )*
# every digit is paired, and not opened and closed on the same atom.
_ORGANIC = ("Br", "Cl", "B", "C", "N", "O", "P", "S", "F", "I", "b", "c", "n", "o", "p", "s")
_BONDS = "-=#/\\:"


def tokenize(text, voc=None):
    """Split a SMILES string into tokens: by longest match against `voc`, or ([...], Br, Cl, single characters) without one."""
    out, i = [], 0
    if voc is not None:
        by_len = sorted(set(voc), key=len, reverse=True)
    while i < len(text):
        if voc is not None:
            tok = next((v for v in by_len if text.startswith(v, i)), None)
            assert tok, f"no vocabulary entry matches {text[i:]!r}"
        elif text[i] == "[":
            tok = text[i:text.index("]", i) + 1]
        else:
            tok = text[i:i + 2] if text[i:i + 2] in ("Br", "Cl") else text[i]
        out.append(tok)
        i += len(tok)
    return out


class _Parser:
    def __init__(self, toks):
        self.toks, self.i, self.open = list(toks), 0, set()

    def peek(self, k=0):
        return self.toks[self.i + k] if self.i + k < len(self.toks) else None

    @staticmethod
    def is_atom(t):
        return t is not None and (t in _ORGANIC or (len(t) > 2 and t[0] == "[" and t[-1] == "]"))

    @staticmethod
    def is_bond(t):
        return t is not None and len(t) == 1 and t in _BONDS

    @staticmethod
    def is_digit(t):
        return t is not None and len(t) == 1 and t in "123456789"

    def branched_atom(self):
        if not self.is_atom(self.peek()):
            return False
        self.i += 1
        here = set()
        while self.is_digit(self.peek()) or (self.is_bond(self.peek()) and self.is_digit(self.peek(1))):
            self.i += 1 if self.is_digit(self.peek()) else 2
            d = self.toks[self.i - 1]
            if d in self.open:
                if d in here:
                    return False                       # C11: opened and closed on the same atom
                self.open.discard(d)
            else:
                self.open.add(d)
                here.add(d)
        while self.peek() == "(":
            self.i += 1
            if self.is_bond(self.peek()):
                self.i += 1
            if not self.chain() or self.peek() != ")":
                return False
            self.i += 1
        return True

    def chain(self):
        if not self.branched_atom():
            return False
        while True:
            t = self.peek()
            if self.is_atom(t):
                ok = self.branched_atom()
            elif self.is_bond(t) or t == ".":
                self.i += 1
                ok = self.branched_atom()
            else:
                return True
            if not ok:
                return False

    def accept(self):
        return self.chain() and self.i == len(self.toks) and not self.open


def parses(toks):
    """toks: token strings (or one string, tokenised without a vocabulary)"""
    return _Parser(tokenize(toks) if isinstance(toks, str) else toks).accept()


ACCEPT = ("C", "C1CC1", "C(=O)C", "C=1CC1", "C.C", "c12cc1C2")
REJECT = ("C()", "C11", "C(C", "C=", "C1C", "(C)", "C)", "C(1)", "C.", "C(C)1", "C(-2)")


def row_text(row, voc, eos):
    """token strings of one returned row between '&' and '$'; None if the row never drew '$'"""
    row = [int(t) for t in row]
    if eos not in row[1:]:
        return None
    return [voc[t] for t in row[1:row.index(eos, 1)]]
