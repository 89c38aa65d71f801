"""CPU restatement (float64) of the forced stochastic-beam rule of include/singa_hip_prefix.h, shared by
tests/test_prefix_cpu.py and tests/test_prefix_gpu.py: `swor_rule.run` with a per-pocket, per-step mask - where a pocket's
forced matrix holds a token in column t + 1, the mask of step t is that single token (`allowed` takes no part), elsewhere it is
`allowed`.  Nothing else differs: the noise is drawn and the conditioning is evaluated as for any mask, which is how the
one-hot column comes out at the parent's G and phi by arithmetic alone.  Philox, the uniform, the hash and the log-sum-exp
are tests/swor_rule.py's."""
import numpy as np

from tests.swor_rule import child_hash, lse, philox, uniform


def step_masks(forced, t, V, allowed=None):
    """bool [B, 1, V]: the effective mask of step t per pocket"""
    forced = np.asarray(forced, np.int64)
    ok = np.ones(V, bool) if allowed is None else np.asarray(allowed).astype(bool)
    out = np.broadcast_to(ok, (len(forced), 1, V)).copy()
    f = forced[:, t + 1]
    for b in np.flatnonzero((f >= 0) & (f < V)):
        out[b, 0] = False
        out[b, 0, f[b]] = True
    return out


def run(table, k, T, seed, streams, sos, eos, pad, tau=1.0, allowed=None, forced=None):
    """`swor_rule.run` (same arguments, same result dict) with `forced` [B, T] integers, a value outside [0, V) = a free
    column; None = all free."""
    table = np.asarray(table, np.float32).astype(np.float64)
    V = table.shape[0]
    B = len(streams)
    forced = np.full((B, T), -1, np.int64) if forced is None else np.asarray(forced, np.int64)
    assert forced.shape == (B, T)
    strm = np.asarray(streams, np.uint64).reshape(B, 1, 1)
    seed = np.asarray(seed, np.uint64)
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
    history = []
    with np.errstate(all="ignore"):
        for t in range(T - 1):
            ok = step_masks(forced, t, V, allowed)
            L = int(np.flatnonzero(np.isfinite(G).any(0)).max()) + 1 if np.isfinite(G).any() else 1
            full = (G, phi, slp, hsh, fin, length, tokens, tlp)
            G, phi, slp, hsh, fin, length, tokens, tlp = (x[:, :L] for x in full)
            z = table[tokens[:, :, t]]
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
            cand[:, :, pad] = np.where(done, G, cand[:, :, pad])
            flat = cand.reshape(B, L * V)
            if L * V < k + 1:
                flat = np.concatenate([flat, np.full((B, k + 1 - L * V), NEG)], 1)
            order = np.argsort(-flat, axis=1, kind="stable")[:, :k + 1]
            vals = np.take_along_axis(flat, order, 1)
            if vals.shape[1] > k:
                d = np.where(np.isfinite(vals[:, k]), vals[:, k - 1] - vals[:, k], np.inf)
                gap = np.minimum(gap, d)
            order, vals = order[:, :k], vals[:, :k]
            par, tok = np.minimum(order // V, L - 1), order % V
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
            history.append((G.copy(), phi.copy()))
    return {"tokens": tokens, "gumbel": G, "prop_logp": phi, "sum_logp": slp, "tok_logp": tlp, "finished": fin, "length": length,
            "hash": hsh, "valid": np.isfinite(G), "gap": gap, "history": history}


def prefix_matrix(prefixes, T, sos):
    """int64 [B, T]: column 0 `sos`, columns 1 .. n the tokens of pocket b's prefix, -1 behind them"""
    out = np.full((len(prefixes), T), -1, np.int64)
    out[:, 0] = sos
    for b, p in enumerate(prefixes):
        out[b, 1:1 + len(p)] = p
    return out


def toy_prefixes(V, lens, seed=0):
    """One prefix of lens[b] tokens per pocket for the toy vocabulary of tests/test_swor_gpu.toy_vocab: drawable tokens that
    are not '$' (ids 3 .. V - 1), drawn once per (V, seed) and cut to length."""
    rs = np.random.RandomState(1000 * seed + V)
    pool = rs.randint(3, V, size=max(lens) if len(lens) else 0)
    return [list(map(int, pool[:n])) for n in lens]


def beam_masks(run, forced):
    """`run.masks()` of a tests/beam_rule.Search with the forced beam rule applied: the live rows of a pocket that is not done
    and whose column t + 1 is forced keep the given token alone - `allowed` and the grammar take no part."""
    masks = run.masks()
    for b in range(run.B):
        f = int(forced[b, run.t + 1])
        if 0 <= f < run.V and not run.done[b]:
            live = run.score[b] > -np.inf
            masks[b, live] = False
            masks[b, live, f] = True
    return masks
