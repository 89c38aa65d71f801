"""CPU restatement (float64) of the token-choice rule of `singa_sample_token` (include/singa_hip.h), shared by
tests/test_sampling_cpu.py and tests/test_sampling_gpu.py, and the teacher-forced oracle evaluation of sampled sequences."""
import numpy as np

EPS = 1e-5          # a decision closer than this to one of its thresholds is ambiguous between fp32 and float64 logits


def logp_bound(V, zmax):
    """fp32 rounding bound of a V-term log-sum-exp on logits of magnitude <= zmax (absolute)."""
    return (V + 8) * 2.0 ** -24 + 2.0 ** -23 * zmax


def choose(z, u, tau, top_k, top_p, allowed=None, eps=0.0, exact_ties=True):
    """-> (token, log-probability, ambiguous).  `ambiguous`: some threshold of the decision (a cumulative F_i against u, the
    gap between the ranks top_k - 1 and top_k, a running mass against top_p; greedy: the gap between the two largest logits)
    is closer than `eps`.  exact_ties: values that are exactly equal are decided by the index rule and are not ambiguous
    (true when both sides read the very same numbers)."""
    z = np.asarray(z, np.float64)
    V = z.shape[0]
    ok = np.ones(V, bool) if allowed is None else np.asarray(allowed).astype(bool)
    m = z.max()
    logp = z - (m + np.log(np.exp(z - m).sum()))
    idx = np.flatnonzero(ok)
    close = (lambda d: d < eps and not (exact_ties and d == 0.0))
    if tau == 0:
        zz = z[idx]
        tok = int(idx[int(np.argmax(zz))])                       # argmax: the first of equals = the lowest index
        top = np.sort(zz)[::-1]
        return tok, float(logp[tok]), bool(len(top) > 1 and close(top[0] - top[1]))
    s = z / tau
    order = sorted((int(i) for i in idx), key=lambda i: (-s[i], i))
    amb = False
    if top_k > 0:
        if top_k < len(order) and close(s[order[top_k - 1]] - s[order[top_k]]):
            amb = True
        order = order[:top_k]
    if top_p < 1:
        sk = s[order]
        q = np.exp(sk - sk.max())
        q = q / q.sum()
        before = np.concatenate([[0.0], np.cumsum(q)[:-1]])
        amb = amb or bool((np.abs(before[1:] - top_p) < eps).any())
        order = [i for i, b in zip(order, before) if b < top_p]
    kept = sorted(order)
    e = np.exp(s[kept] - s[kept].max())
    F = np.cumsum(e) / e.sum()
    amb = amb or bool((np.abs(F[:-1] - u) < eps).any())          # the last kept token is the fall-back: no threshold of its own
    hit = np.flatnonzero(F > u)
    tok = kept[int(hit[0])] if len(hit) else kept[-1]
    return tok, float(logp[tok]), amb


def brute_force(z, u, tau, top_k, top_p, allowed=None):
    """The rule read literally, with explicit loops (tiny V only): the token."""
    V = len(z)
    ok = [True] * V if allowed is None else [bool(a) for a in allowed]
    if tau == 0:
        best = None
        for i in range(V):
            if ok[i] and (best is None or z[i] > z[best]):
                best = i
        return best
    s = [float(z[i]) / tau for i in range(V)]
    before = lambda j, i: s[j] > s[i] or (s[j] == s[i] and j < i)          # j is ranked before i
    rank = [sum(1 for j in range(V) if ok[j] and j != i and before(j, i)) for i in range(V)]
    keep = [ok[i] and (top_k == 0 or rank[i] < top_k) for i in range(V)]
    mx = max(s[i] for i in range(V) if keep[i])
    if top_p < 1:
        tot = sum(np.exp(s[i] - mx) for i in range(V) if keep[i])
        mass = [sum(np.exp(s[j] - mx) / tot for j in range(V) if keep[j] and rank[j] < rank[i]) for i in range(V)]
        keep = [keep[i] and mass[i] < top_p for i in range(V)]
    tot = sum(np.exp(s[i] - mx) for i in range(V) if keep[i])
    run, last = 0.0, None
    for i in range(V):
        if keep[i]:
            run += np.exp(s[i] - mx)
            last = i
            if run / tot > u:
                return i
    return last


def oracle_logits(sd, voc, tokens, feat, pos, batch, lap, knn, prop, batch_size):
    """The CPU oracle's logits for every decision of the sampled `tokens` [rows, T], teacher-forced: [rows, T - 1, V], entry t
    is what column t + 1 was drawn from.  Rows are pocket-major.  No key is treated as padding: to the KV-cached decoder a
    '^' inside a live prefix is a token like any other, and what follows a finished row is never compared."""
    import torch

    from oracle import singa_oracle as SO
    sd = dict(sd)
    sd.setdefault("model.decoder.pos_emb.pe", SO.positional_table(sd["model.decoder.mol_emb.weight"].shape[1]))
    tokens = torch.as_tensor(tokens).long()
    per = tokens.shape[0] // batch_size
    with torch.no_grad():
        enc, pad, _ = SO.encoder1_forward(sd, "model.", feat, pos, batch, lap, knn, batch_size)
        out = SO.decoder_forward(sd, "model.", tokens[:, :-1], prop, enc.repeat_interleave(per, 0),
                                 pad.repeat_interleave(per, 0), pad_id=-1)
    return out[:, 1:].double().numpy()


def check_against_oracle(tokens, uniforms, logits, eos, tau, top_k, top_p, eps=EPS, allowed=None):
    """Every live decision of `tokens` [rows, T] against the rule applied to the oracle's `logits` [rows, T - 1, V] and the
    uniforms [T, rows] the kernel read; `allowed` [V] (0 = never drawn) as handed to the kernel.  -> dict: live decisions,
    ambiguous ones, unambiguous mismatches [(row, t, got, want)], the oracle's log-probability of every drawn token [rows, T]
    (0 where the row was finished), lengths, and `checked` [rows, T] bool: column c holds True where the token of column c
    was a live, unambiguous decision, i.e. one that was compared."""
    tokens, uniforms = np.asarray(tokens), np.asarray(uniforms, np.float64)
    R, T = tokens.shape
    live = amb = 0
    bad, lp = [], np.zeros((R, T))
    lengths = np.zeros(R, np.int64)
    checked = np.zeros((R, T), bool)
    for r in range(R):
        for t in range(T - 1):
            want, _, a = choose(logits[r, t], uniforms[t, r], tau, top_k, top_p, allowed, eps=eps, exact_ties=False)
            got = int(tokens[r, t + 1])
            z = logits[r, t]
            lp[r, t + 1] = z[got] - (z.max() + np.log(np.exp(z - z.max()).sum()))
            live += 1
            lengths[r] += 1
            amb += a
            checked[r, t + 1] = not a
            if not a and got != want:
                bad.append((r, t, got, want))
            if got == eos:
                break
    return {"live": live, "ambiguous": amb, "bad": bad, "logp": lp, "lengths": lengths, "checked": checked}
