"""Helper (no tests): forced tokens against the CPU restatements.  Wraps tests/sampling_rule.py (`choose`, `oracle_logits`) for
rows whose first columns are given instead of drawn: a forced column is no decision - its token is compared with the matrix
and only its log-probability with the oracle - while every free column is a decision like any other.  Also the numpy rank of
a token among raw logits, and prefixes spelled from the shipped vocabulary.  Shared by tests/test_forced_cpu.py and
tests/test_forced_gpu.py."""
import numpy as np

from tests.sampling_rule import EPS, choose, oracle_logits  # noqa: F401  (re-exported)

# valid under the rule of include/singa_hip_gen.h, and completable: 0, 1, 5 and 12 tokens
PREFIXES = ("", "C", "c1ccc", "CC(=O)Nc1ccc")
PREFIX_TOKENS = (0, 1, 5, 12)


def rank_of(z, tok):
    """number of j with z_j > z_tok, or z_j == z_tok and j < tok: on the very numbers given, ties decided by index"""
    z = np.asarray(z)
    return int((z > z[tok]).sum() + (z[:tok] == z[tok]).sum())


def is_forced(forced, V):
    forced = np.asarray(forced)
    return (forced >= 0) & (forced < V)


def check_forced_against_oracle(tokens, forced, uniforms, logits, eos, tau, top_k, top_p, eps=EPS, allowed=None):
    """`sampling_rule.check_against_oracle` for rows with forced columns.  tokens, forced [rows, T]; logits [rows, T - 1, V] the
    oracle's, teacher-forced on `tokens`; uniforms [T, rows].  -> dict: `free` (live free decisions), `ambiguous` (of them),
    `bad` [(row, t, got, want)] unambiguous mismatches among the free decisions, `forced_bad` [(row, column)] forced columns
    whose token is not the given one, `logp` [rows, T] the oracle's log-probability of every live token (forced or free),
    `lengths`, `forced_live` [rows, T] bool: live forced columns."""
    tokens, forced, uniforms = np.asarray(tokens), np.asarray(forced), np.asarray(uniforms, np.float64)
    R, T = tokens.shape
    V = logits.shape[-1]
    given = is_forced(forced, V)
    free = amb = 0
    bad, fbad, lp = [], [], np.zeros((R, T))
    lengths = np.zeros(R, np.int64)
    flive = np.zeros((R, T), bool)
    for r in range(R):
        for t in range(T - 1):
            z = logits[r, t]
            got = int(tokens[r, t + 1])
            lp[r, t + 1] = z[got] - (z.max() + np.log(np.exp(z - z.max()).sum()))
            lengths[r] += 1
            if given[r, t + 1]:
                flive[r, t + 1] = True
                if got != int(forced[r, t + 1]):
                    fbad.append((r, t + 1))
            else:
                want, _, a = choose(z, uniforms[t, r], tau, top_k, top_p, allowed, eps=eps, exact_ties=False)
                free += 1
                amb += a
                if not a and got != want:
                    bad.append((r, t, got, want))
            if got == eos:
                break
    return {"free": free, "ambiguous": amb, "bad": bad, "forced_bad": fbad, "logp": lp, "lengths": lengths, "forced_live": flive}
