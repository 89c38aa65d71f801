"""The rule of include/singa_hip_beam.h restated in numpy and plain Python - expand, select, hypotheses - for the tests of the
device beam search.  The masks are those of tests/grammar_rule.py and tests/valence_rule.py; the log-softmax is evaluated in
float32 with the expressions the header names.  Nothing here imports the package's own `_select` or `BeamHypotheses`:
tests/test_beam_device_cpu.py pins this restatement to them."""
import numpy as np

from tests import grammar_rule as G
from tests import valence_rule as VR

NEG = np.float32(-np.inf)


def log_probs(z):
    """z [..., V] f32 -> z - lse in f32, lse = zmax + log(sum exp(z - zmax))"""
    z = np.asarray(z, np.float32)
    zmax = z.max(-1, keepdims=True)
    lse = zmax + np.log(np.exp(z - zmax, dtype=np.float32).sum(-1, keepdims=True, dtype=np.float32), dtype=np.float32)
    return (z - lse).astype(np.float32)


class Hypotheses:
    """`BeamHypotheses` restated: entries [score f64, sum f32, tokens, stamp] in the order stored"""

    def __init__(self, k):
        self.k, self.items, self.worst, self.dropped = k, [], 1e9, 0

    def add(self, tokens, total, denom, stamp):
        score = float(total) / denom
        if len(self.items) >= self.k and score <= self.worst:
            return False
        self.items.append([score, np.float32(total), np.array(tokens, np.int64), stamp])
        if len(self.items) > self.k:
            drop = min(range(len(self.items)), key=lambda i: (self.items[i][0], i))
            del self.items[drop]
            self.dropped += 1
            self.worst = min(it[0] for it in self.items)
        else:
            self.worst = min(score, self.worst)
        return True

    def is_done(self, best, denom):
        return len(self.items) >= self.k and self.worst >= float(best) / denom


class Search:
    """The state of a run for B pockets of k slots.  `cls` (class bytes) turns the SMILES rule on, `cls` and `cap` the valence
    rule; `allowed` [V] removes tokens.  `step(logits)` is expand, then select; after it `parent` / `token` [B, k] hold the
    selection (-1 for a dead slot), `ranked` [B] the ranked candidate values the walk saw."""

    def __init__(self, B, k, V, T, sos, eos, pad, length_penalty=0.7, allowed=None, cls=None, cap=None):
        self.B, self.k, self.V, self.T, self.eos, self.pad, self.t = B, k, V, T, eos, pad, 0
        self.len_pow = [1.0] + [float(n ** length_penalty) for n in range(1, T + 1)]
        self.allowed = np.ones(V, bool) if allowed is None else np.asarray(allowed).astype(bool)
        self.cls = None if cls is None else np.asarray(cls, np.int64)
        self.cap = None if cap is None else np.asarray(cap, np.int64) & 7
        self.score = np.full((B, k), NEG, np.float32)
        self.score[:, 0] = 0
        self.length = np.zeros((B, k), np.int32)
        self.tokens = np.full((B, k, T), pad, np.int64)
        self.tokens[:, :, 0] = sos
        self.next = np.full((B, k), sos, np.int64)
        self.src = np.zeros((B, k), np.int64)
        self.gstate = np.full((B, k), G.FRESH, np.int64)
        self.vstate = np.zeros((B, k, 2), np.int64)
        self.hyps = [Hypotheses(k) for _ in range(B)]
        self.done = np.zeros(B, bool)
        self.done_step = [None] * B
        self.live = np.ones(B, np.int32)
        self.parent, self.token = np.full((B, k), -1), np.full((B, k), -1)
        self.ranked = [np.zeros(0, np.float32)] * B

    def mask(self, b, i):
        rem = self.T - 2 - self.t
        ok = self.allowed.copy()
        if self.cls is not None and self.cap is not None:
            ok &= VR.allows(self.gstate[b, i], self.vstate[b, i, 0], self.vstate[b, i, 1], self.cls, self.cap, rem)
        elif self.cls is not None:
            ok &= G.allows(np.full(self.V, self.gstate[b, i]), self.cls, np.full(self.V, rem))
        return ok

    def after(self, b, i, v):
        """the state words of slot (b, i) after token v"""
        if self.cls is None:
            return self.gstate[b, i], self.vstate[b, i]
        if self.cap is None:
            return int(G.transition(self.gstate[b, i], self.cls[v])), self.vstate[b, i]
        st, v0, v1 = VR.transition(self.gstate[b, i], self.vstate[b, i, 0], self.vstate[b, i, 1], self.cls[v], self.cap[v])
        return int(st), np.array([int(v0), int(v1)], np.int64)

    def masks(self):
        """bool [B, k, V]: what may follow every live slot of a pocket that is not done at this step; nothing elsewhere"""
        ok = np.zeros((self.B, self.k, self.V), bool)
        for b in range(self.B):
            for i in range(self.k):
                if not self.done[b] and self.score[b, i] > NEG:
                    ok[b, i] = self.mask(b, i)
        return ok

    def expand(self, logits, masks=None):
        lp = log_probs(np.asarray(logits, np.float32).reshape(self.B, self.k, self.V))
        ok = self.masks() if masks is None else masks
        return np.where(ok, (self.score[:, :, None] + lp).astype(np.float32), NEG)

    def select(self, cand):
        k, V, t = self.k, self.V, self.t
        for b in range(self.B):
            if self.done[b]:
                continue
            flat = cand[b].reshape(-1)
            order = np.lexsort((np.arange(k * V), -flat.astype(np.float64)))      # value down, then slot, then token
            order = [int(f) for f in order if flat[f] > NEG][:2 * k]
            self.ranked[b] = flat[order]
            denom = self.len_pow[t + 1]
            kept, done = [], False
            for rank, f in enumerate(order):
                i, v = divmod(f, V)
                if v == self.eos:
                    if rank >= k:
                        continue
                    self.hyps[b].add(self.tokens[b, i, :t + 1], flat[f], denom, t * 2 * k + rank)
                else:
                    kept.append((i, v, flat[f]))
                if len(kept) == k:
                    break
                done = done or self.hyps[b].is_done(flat[order[0]], denom)
            score, length, tokens = self.score[b].copy(), self.length[b].copy(), self.tokens[b].copy()     # the parents stay
            gstate, vstate = self.gstate[b].copy(), self.vstate[b].copy()                                  # readable meanwhile
            self.parent[b], self.token[b] = -1, -1
            for j in range(k):
                if j < len(kept):
                    i, v, s = kept[j]
                    score[j], length[j] = s, self.length[b, i] + 1
                    tokens[j, :t + 1], tokens[j, t + 1] = self.tokens[b, i, :t + 1], v
                    gstate[j], vstate[j] = self.after(b, i, v)
                    self.next[b, j], self.src[b, j] = v, b * k + i
                    self.parent[b, j], self.token[b, j] = i, v
                else:                                                              # dead: tokens, length and state words kept
                    score[j] = NEG
                    self.next[b, j], self.src[b, j] = self.pad, b * k + j
            self.score[b], self.length[b], self.tokens[b], self.gstate[b], self.vstate[b] = score, length, tokens, gstate, vstate
            if done:
                self.done[b], self.done_step[b] = True, t
            self.live[b] = 0 if done else len(kept)

    def snapshot(self):
        """copies of everything a step leaves, the hypotheses as lists of (score, sum, tokens, stamp) in the order stored"""
        names = ("score", "length", "tokens", "next", "src", "gstate", "vstate", "done", "live", "parent", "token")
        out = {n: getattr(self, n).copy() for n in names}
        out.update(hyps=[[tuple(it) for it in h.items] for h in self.hyps], worst=[h.worst for h in self.hyps], pad=self.pad,
                   ranked=[len(r) for r in self.ranked])
        return out

    def step(self, logits):
        self.select(self.expand(logits))
        self.t += 1

    def finish(self):
        """BS:141-149: a pocket that is not done adds its live slots"""
        for b in range(self.B):
            if not self.done[b]:
                for i in range(self.k):
                    if self.score[b, i] > NEG:
                        n = self.length[b, i] + 1
                        self.hyps[b].add(self.tokens[b, i, :n], self.score[b, i], self.len_pow[n], -1)
