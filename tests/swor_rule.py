"""CPU restatement (float64) of the rule of include/singa_hip_swor.h - stochastic beam search, sampling without replacement -
shared by tests/test_swor_cpu.py and tests/test_swor_gpu.py.  Philox4x32-10, the uniform and the prefix hash are written in
numpy integers; everything behind them is float64.  The model is a first-order Markov toy: logits = table[previous token]."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(seed, hash_, v, stream):
    """First output word of Philox4x32-10, key = the 64-bit `seed`, counter = (hash lo, hash hi, v, stream); arrays broadcast."""
    seed, hash_ = np.asarray(seed, np.uint64), np.asarray(hash_, np.uint64)
    shape = np.broadcast(seed, hash_, np.asarray(v), np.asarray(stream)).shape
    c = [np.broadcast_to(x, shape).astype(np.uint64) for x in (hash_ & LOW, hash_ >> S32, np.asarray(v, np.uint64) & LOW,
                                                              np.asarray(stream, np.uint64) & LOW)]
    k0, k1 = np.broadcast_to(seed & LOW, shape).astype(np.uint64), np.broadcast_to(seed >> S32, shape).astype(np.uint64)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & LOW, (p0 >> S32) ^ c[3] ^ k1, p0 & LOW]
        k0, k1 = (k0 + np.uint64(W0)) & LOW, (k1 + np.uint64(W1)) & LOW
    return c[0].astype(np.uint32)


def uniform(x):
    """u = ((x >> 8) + 0.5) * 2^-24 in float32 arithmetic; a result that rounds to 1 becomes 1 - 2^-24."""
    u = ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.where(u < np.float32(1), u, np.float32(1) - np.float32(2.0 ** -24)).astype(np.float32)


def child_hash(h, v):
    """splitmix64's finaliser of h + (v + 1) * 0x9E3779B97F4A7C15 (mod 2^64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(h, np.uint64) + (np.asarray(v, np.int64) + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def lse(x):
    m = x.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return m + np.log(np.exp(x - m).sum(-1, keepdims=True))


def run(table, k, T, seed, streams, sos, eos, pad, tau=1.0, allowed=None):
    """The rule, step by step, for len(streams) pockets of k slots on the toy model `table` [V, V] (float32 logits, row =
    previous token).  -> dict of the final slots in the rule's order: tokens [B, k, T], gumbel, prop_logp, sum_logp [B, k]
    (float64; -inf / 0 for dead slots), tok_logp [B, k, T], finished, length, hash, valid, and `gap` [B]: the smallest
    difference, over the steps, between the k-th and the (k + 1)-th best candidate of the pocket (inf where there is no
    (k + 1)-th): a run whose gap is below the device's error in g~ is ambiguous."""
    table = np.asarray(table, np.float32).astype(np.float64)
    V = table.shape[0]
    B = len(streams)
    ok = np.ones(V, bool) if allowed is None else np.asarray(allowed).astype(bool)
    strm = np.asarray(streams, np.uint64).reshape(B, 1, 1)
    seed = np.asarray(seed, np.uint64)                                               # one seed, or one per pocket
    seed = seed.reshape(B, 1, 1) if seed.ndim else seed
    NEG = -np.inf
    G, phi = np.full((B, k), NEG), np.full((B, k), NEG)
    G[:, 0] = phi[:, 0] = 0.0
    slp, hsh = np.zeros((B, k)), np.zeros((B, k), np.uint64)
    fin, length = np.zeros((B, k), bool), np.zeros((B, k), np.int64)
    tokens, tlp = np.full((B, k, T), pad, np.int64), np.zeros((B, k, T))
    tokens[:, :, 0] = sos
    gap = np.full(B, np.inf)
    bi = np.arange(B)[:, None]
    with np.errstate(all="ignore"):
        for t in range(T - 1):
            L = int(np.flatnonzero(np.isfinite(G).any(0)).max()) + 1 if np.isfinite(G).any() else 1   # dead slots trail
            full = (G, phi, slp, hsh, fin, length, tokens, tlp)
            G, phi, slp, hsh, fin, length, tokens, tlp = (x[:, :L] for x in full)    # parents: the first L slots
            z = table[tokens[:, :, t]]                                               # [B, L, V]
            lp = z - lse(z)
            s = np.where(ok, z / tau, NEG)
            q = s - lse(s)
            u = uniform(philox(seed, hsh[:, :, None], np.arange(V).reshape(1, 1, V), strm)).astype(np.float64)
            g = np.where(ok, phi[:, :, None] + q - np.log(-np.log(u)), NEG)
            Z = g.max(-1, keepdims=True)
            a = G[:, :, None] - g + np.log1p(-np.exp(g - Z))
            gt = G[:, :, None] - np.maximum(a, 0.0) - np.log1p(np.exp(-np.abs(a)))
            live = np.isfinite(G) & ~fin
            cand = np.where(live[:, :, None] & ok, gt, NEG)
            done = np.isfinite(G) & fin
            cand[:, :, pad] = np.where(done, G, cand[:, :, pad])                      # a finished parent: itself, emitting pad
            flat = cand.reshape(B, L * V)
            if L * V < k + 1:
                flat = np.concatenate([flat, np.full((B, k + 1 - L * V), NEG)], 1)
            order = np.argsort(-flat, axis=1, kind="stable")[:, :k + 1]               # ties: lower parent, then lower token
            vals = np.take_along_axis(flat, order, 1)
            if vals.shape[1] > k:
                d = np.where(np.isfinite(vals[:, k]), vals[:, k - 1] - vals[:, k], np.inf)
                gap = np.minimum(gap, d)
            order, vals = order[:, :k], vals[:, :k]
            par, tok = np.minimum(order // V, L - 1), order % V                       # (padding entries are dead: -inf)
            alive = np.isfinite(vals)
            pf = fin[bi, par]
            nG = np.where(alive, vals, NEG)
            nphi = np.where(alive, np.where(pf, phi[bi, par], (phi[:, :, None] + q)[bi, par, tok]), NEG)
            step_lp = np.where(pf, 0.0, lp[bi, par, tok])
            nslp = np.where(alive, slp[bi, par] + step_lp, 0.0)
            nh = np.where(alive, np.where(pf, hsh[bi, par], child_hash(hsh[bi, par], tok)), np.uint64(0))
            nfin = alive & (pf | (tok == eos))
            nlen = np.where(alive, length[bi, par] + ~pf, 0)
            ntok, ntlp = tokens[bi, par].copy(), tlp[bi, par].copy()
            ntok[:, :, t + 1] = np.where(pf, pad, tok)
            ntlp[:, :, t + 1] = step_lp
            ntok[~alive, 1:] = pad
            ntlp[~alive] = 0.0
            G, phi, slp, hsh, fin, length, tokens, tlp = nG, nphi, nslp, nh, nfin, nlen, ntok, ntlp
    return {"tokens": tokens, "gumbel": G, "prop_logp": phi, "sum_logp": slp, "tok_logp": tlp, "finished": fin, "length": length,
            "hash": hsh, "valid": np.isfinite(G), "gap": gap}


def toy_table(V, seed, sos, eos, pad, scale=2.0, eos_rows=0.3):
    """A Markov table [V, V] float32: normal logits of spread `scale`; after a fraction `eos_rows` of the tokens '$' is
    the likeliest continuation, so that rows finish at different steps."""
    rs = np.random.RandomState(seed)
    table = (rs.randn(V, V) * scale).astype(np.float32)
    table[rs.rand(V) < eos_rows, eos] = np.float32(2.0 * scale)
    return table


def plackett_luce_inclusion(p, k=2):
    """Inclusion probabilities of sampling k = 2 of len(p) items without replacement, probabilities p."""
    assert k == 2
    p = np.asarray(p, np.float64)
    return np.array([p[i] + sum(p[j] * p[i] / (1 - p[j]) for j in range(len(p)) if j != i) for i in range(len(p))])
