"""Sampled generation, the part that runs without a GPU: the argument errors of `singa_sample_token` through the built
library, the float64 restatement of its rule (tests/sampling_rule.py) against a literal brute-force reading on tiny
vocabularies, and `sample` / `ops.sample_token` refusing CPU tensors.  The kernel itself uses cross-lane operations (wave
scans, lane broadcasts) and is therefore, like `singa_lap_pe`, not part of the sequential emulation build: it is compared
with the restatement on the GPU (tests/test_sampling_gpu.py)."""
import ctypes

import numpy as np
import pytest

from tests.sampling_rule import brute_force, check_against_oracle, choose


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_sample_token_argument_errors_without_gpu(lib):
    """Validation happens before any HIP call: SINGA_E_NULL = -1, SINGA_E_SHAPE as the other entry points return it."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks
    shape = lib.singa_edge_mlp_fwd(*([p] * 11), 1, 1, 1, 1, None)       # a known SINGA_E_SHAPE
    assert shape not in (0, -1)

    def call(V=116, tau=1.0, top_k=0, top_p=1.0, T=8, eos=3, pad=4, logits=p, live=p):
        return lib.singa_sample_token(logits, p, None, p, 2, 4, V, T, tau, top_k, top_p, eos, pad, p, p, p, p, p, live, None, None)

    assert call(logits=None) == -1 and call(live=None) == -1
    assert b"sample_token" in lib.singa_last_error_string()
    for bad in (dict(V=0), dict(V=1025), dict(V=-3), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(tau=-0.5),
                dict(top_k=-1), dict(T=1), dict(eos=116), dict(pad=-1), dict(tau=float("nan")), dict(top_p=float("nan"))):
        assert call(**bad) == shape, bad
    assert b"sample_token" in lib.singa_last_error_string()
    # valid arguments and no rows: nothing to launch
    assert lib.singa_sample_token(p, p, None, p, 2, 0, 116, 8, 1.0, 0, 1.0, 3, 4, p, p, p, p, p, p, None, None) == 0
    assert lib.singa_sample_token(p, p, None, p, 2, 0, 1024, 8, 0.0, 7, 1e-6, 3, 4, p, p, p, p, p, p, p, None) == 0


NAN = float("nan")
# (entry point, the arguments that differ from a valid call, return code, text of singa_last_error_string() behind "<entry>: "),
# recorded from the library as it was when each entry point carried its own checks: one bad argument at a time, then pairs,
# which pin the order of the checks.  Pointers: True = some address, None = null, "misaligned" = that address + 4.
BAD_ARGUMENTS = [
    ("sample_token", dict(logits=None), -1, "null pointer"),
    ("sample_token", dict(live=None), -1, "null pointer"),
    ("sample_token", dict(V=0), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token", dict(V=1025), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token", dict(tau=-0.5), -3, "temperature must be >= 0"),
    ("sample_token", dict(tau=NAN), -3, "temperature must be >= 0"),
    ("sample_token", dict(top_k=-1), -3, "top_k must be >= 0 (0 = off)"),
    ("sample_token", dict(top_p=0.0), -3, "top_p must be in (0, 1]"),
    ("sample_token", dict(top_p=1.5), -3, "top_p must be in (0, 1]"),
    ("sample_token", dict(top_p=NAN), -3, "top_p must be in (0, 1]"),
    ("sample_token", dict(T=1), -3, "T >= 2 columns, eos / pad inside the vocabulary"),
    ("sample_token", dict(eos=116), -3, "T >= 2 columns, eos / pad inside the vocabulary"),
    ("sample_token", dict(eos=-1), -3, "T >= 2 columns, eos / pad inside the vocabulary"),
    ("sample_token", dict(pad=116), -3, "T >= 2 columns, eos / pad inside the vocabulary"),
    ("sample_token", dict(pad=-1), -3, "T >= 2 columns, eos / pad inside the vocabulary"),
    ("sample_token_grammar", dict(logits=None), -1, "null pointer"),
    ("sample_token_grammar", dict(live=None), -1, "null pointer"),
    ("sample_token_grammar", dict(cls=None), -1, "null pointer"),
    ("sample_token_grammar", dict(gstate=None), -1, "null pointer"),
    ("sample_token_grammar", dict(V=0), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token_grammar", dict(V=1025), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token_grammar", dict(tau=-0.5), -3, "temperature must be >= 0"),
    ("sample_token_grammar", dict(tau=NAN), -3, "temperature must be >= 0"),
    ("sample_token_grammar", dict(top_k=-1), -3, "top_k must be >= 0 (0 = off)"),
    ("sample_token_grammar", dict(top_p=0.0), -3, "top_p must be in (0, 1]"),
    ("sample_token_grammar", dict(top_p=1.5), -3, "top_p must be in (0, 1]"),
    ("sample_token_grammar", dict(top_p=NAN), -3, "top_p must be in (0, 1]"),
    ("sample_token_grammar", dict(T=2), -3, "T >= 3 columns, eos / pad inside the vocabulary"),
    ("sample_token_grammar", dict(eos=116), -3, "T >= 3 columns, eos / pad inside the vocabulary"),
    ("sample_token_grammar", dict(eos=-1), -3, "T >= 3 columns, eos / pad inside the vocabulary"),
    ("sample_token_grammar", dict(pad=116), -3, "T >= 3 columns, eos / pad inside the vocabulary"),
    ("sample_token_grammar", dict(pad=-1), -3, "T >= 3 columns, eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(logits=None), -1, "null pointer"),
    ("sample_token_forced", dict(live=None), -1, "null pointer"),
    ("sample_token_forced", dict(forced=None), -1, "null pointer"),
    ("sample_token_forced", dict(cls=True), -1, "cls and gstate go together (allowed_logp only with them)"),
    ("sample_token_forced", dict(gstate=True), -1, "cls and gstate go together (allowed_logp only with them)"),
    ("sample_token_forced", dict(alp=True), -1, "cls and gstate go together (allowed_logp only with them)"),
    ("sample_token_forced", dict(V=0), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token_forced", dict(V=1025), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token_forced", dict(tau=-0.5), -3, "temperature must be >= 0"),
    ("sample_token_forced", dict(tau=NAN), -3, "temperature must be >= 0"),
    ("sample_token_forced", dict(top_k=-1), -3, "top_k must be >= 0 (0 = off)"),
    ("sample_token_forced", dict(top_p=0.0), -3, "top_p must be in (0, 1]"),
    ("sample_token_forced", dict(top_p=1.5), -3, "top_p must be in (0, 1]"),
    ("sample_token_forced", dict(top_p=NAN), -3, "top_p must be in (0, 1]"),
    ("sample_token_forced", dict(T=1), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(eos=116), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(eos=-1), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(pad=116), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(pad=-1), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("sample_token_forced", dict(T=2, cls=True, gstate=True), -3, "T >= 2 columns (3 under the grammar), eos / pad inside the vocabulary"),
    ("swor_expand", dict(cand=None), -1, "null pointer"),
    ("swor_expand", dict(cls=True), -1, "cls and gstate go together"),
    ("swor_expand", dict(gstate=True), -1, "cls and gstate go together"),
    ("swor_expand", dict(V=0), -3, "vocabulary of 1..1024 tokens"),
    ("swor_expand", dict(V=1025), -3, "vocabulary of 1..1024 tokens"),
    ("swor_expand", dict(k=0), -3, "1..2048 slots per pocket"),
    ("swor_expand", dict(k=2049, rows=2049), -3, "1..2048 slots per pocket"),
    ("swor_expand", dict(rows=5), -3, "rows must be pockets x slots"),
    ("swor_expand", dict(T=1), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_expand", dict(T=2, cls=True, gstate=True), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_expand", dict(pad=116), -3, "eos / pad inside the vocabulary"),
    ("swor_expand", dict(pad=-1), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(cand=None), -1, "null pointer"),
    ("swor_select", dict(cls=True), -1, "cls and gstate go together"),
    ("swor_select", dict(gstate=True), -1, "cls and gstate go together"),
    ("swor_select", dict(V=0), -3, "vocabulary of 1..1024 tokens"),
    ("swor_select", dict(V=1025), -3, "vocabulary of 1..1024 tokens"),
    ("swor_select", dict(k=0), -3, "1..2048 slots per pocket"),
    ("swor_select", dict(k=2049, rows=2049), -3, "1..2048 slots per pocket"),
    ("swor_select", dict(rows=5), -3, "rows must be pockets x slots"),
    ("swor_select", dict(T=1), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_select", dict(T=2, cls=True, gstate=True), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_select", dict(pad=116), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(pad=-1), -3, "eos / pad inside the vocabulary"),
    ("swor_expand", dict(logits=None), -1, "null pointer"),
    ("swor_expand", dict(streams=None), -1, "null pointer"),
    ("swor_expand", dict(tau=0.0), -3, "temperature must be > 0"),
    ("swor_expand", dict(tau=-1.0), -3, "temperature must be > 0"),
    ("swor_expand", dict(tau=NAN), -3, "temperature must be > 0"),
    ("swor_select", dict(work=None), -1, "null pointer"),
    ("swor_select", dict(live=None), -1, "null pointer"),
    ("swor_select", dict(eos=116), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(eos=-1), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(work="misaligned"), -3, "work must be 16-byte aligned"),
    ("sample_token", dict(logits=None, V=0), -1, "null pointer"),
    ("sample_token", dict(V=0, tau=-1.0), -3, "vocabulary of 1..1024 tokens"),
    ("sample_token", dict(tau=NAN, top_k=-1), -3, "temperature must be >= 0"),
    ("sample_token", dict(top_k=-1, top_p=0.0), -3, "top_k must be >= 0 (0 = off)"),
    ("sample_token", dict(top_p=1.5, T=1), -3, "top_p must be in (0, 1]"),
    ("sample_token_grammar", dict(cls=None, V=1025), -1, "null pointer"),
    ("sample_token_grammar", dict(top_p=1.5, T=2), -3, "top_p must be in (0, 1]"),
    ("sample_token_forced", dict(forced=None, cls=True), -1, "null pointer"),
    ("sample_token_forced", dict(cls=True, V=0), -1, "cls and gstate go together (allowed_logp only with them)"),
    ("sample_token_forced", dict(V=0, T=1), -3, "vocabulary of 1..1024 tokens"),
    ("swor_expand", dict(logits=None, cls=True), -1, "null pointer"),
    ("swor_expand", dict(cls=True, V=0), -1, "cls and gstate go together"),
    ("swor_expand", dict(V=0, k=0), -3, "vocabulary of 1..1024 tokens"),
    ("swor_expand", dict(k=0, rows=5), -3, "1..2048 slots per pocket"),
    ("swor_expand", dict(rows=5, T=1), -3, "rows must be pockets x slots"),
    ("swor_expand", dict(T=1, pad=-1), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_expand", dict(pad=-1, tau=0.0), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(cand=None, gstate=True), -1, "null pointer"),
    ("swor_select", dict(gstate=True, k=0), -1, "cls and gstate go together"),
    ("swor_select", dict(T=1, eos=-1), -3, "T >= 2 columns (3 under the grammar)"),
    ("swor_select", dict(eos=-1, work="misaligned"), -3, "eos / pad inside the vocabulary"),
    ("swor_select", dict(V=1025, work="misaligned"), -3, "vocabulary of 1..1024 tokens"),
]


@pytest.mark.parametrize("entry,bad,code,text", BAD_ARGUMENTS, ids=[f"{e}-{i}" for i, (e, *_) in enumerate(BAD_ARGUMENTS)])
def test_generation_entry_points_report_bad_arguments_as_recorded(lib, entry, bad, code, text):
    """The five entry points that validate a token choice or a selection step - `singa_sample_token`, `_grammar`, `_forced`,
    `singa_swor_expand`, `singa_swor_select` - return the same code and leave the same text, byte for byte, for every tuple of
    the table.  No pointer is dereferenced: every call fails its checks."""
    buf = (ctypes.c_char * 80)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    a = dict(V=116, tau=1.0, top_k=0, top_p=1.0, T=8, eos=3, pad=4, rows=4, k=2, logits=True, live=True, cand=True, streams=True,
             work=True, cls=entry == "sample_token_grammar", gstate=entry == "sample_token_grammar", alp=None, forced=True, rank=None)
    a.update(bad)
    q = {n: p if a[n] is True else ctypes.c_void_p(p.value + 4) if a[n] == "misaligned" else None
         for n in ("logits", "live", "cand", "streams", "work", "cls", "gstate", "alp", "forced", "rank")}
    choice = (a["rows"], a["V"], a["T"], a["tau"], a["top_k"], a["top_p"], a["eos"], a["pad"], p, p, p, p, p, q["live"], None)
    if entry == "sample_token":
        got = lib.singa_sample_token(q["logits"], p, None, p, 2, *choice, None)
    elif entry == "sample_token_grammar":
        got = lib.singa_sample_token_grammar(q["logits"], p, None, q["cls"], p, 2, *choice, q["gstate"], q["alp"], None)
    elif entry == "sample_token_forced":
        got = lib.singa_sample_token_forced(q["logits"], p, None, q["cls"], p, 2, *choice, q["gstate"], q["alp"], q["forced"],
                                            q["rank"], None)
    elif entry == "swor_expand":
        got = lib.singa_swor_expand(q["logits"], None, q["cls"], p, 1, a["rows"], a["k"], a["V"], a["T"], a["tau"], 7, q["streams"],
                                    a["pad"], p, p, p, p, q["gstate"], q["cand"], p, p, None)
    else:
        assert entry == "swor_select"
        got = lib.singa_swor_select(q["cand"], p, p, q["cls"], p, 1, a["rows"], a["k"], a["V"], a["T"], a["eos"], a["pad"], p, p, p, p,
                                    p, p, q["gstate"], p, p, p, p, q["live"], q["work"], None)
    assert (got, lib.singa_last_error_string()) == (code, f"{entry}: {text}".encode())


def test_restatement_matches_brute_force_on_tiny_vocabularies():
    rs = np.random.RandomState(0)
    n = 0
    for V in (1, 2, 3, 5, 6):
        for _ in range(120):
            z = rs.uniform(-3, 3, V)
            if rs.rand() < 0.4 and V > 1:                 # exact ties
                z[rs.randint(V)] = z[rs.randint(V)]
            allowed = None
            if rs.rand() < 0.3 and V > 1:
                allowed = rs.rand(V) < 0.6
                allowed[rs.randint(V)] = True
            tau = [0.0, 0.5, 1.0, 2.0][rs.randint(4)]
            top_k = [0, 1, 2, V, V + 3][rs.randint(5)]
            top_p = [1.0, 0.9, 0.5, 1e-6][rs.randint(4)]
            u = [0.0, 1 - 2.0 ** -24, rs.rand(), rs.rand()][rs.randint(4)]
            tok, logp, _ = choose(z, u, tau, top_k, top_p, allowed)
            assert tok == brute_force(z, u, tau, top_k, top_p, allowed), (V, z, u, tau, top_k, top_p, allowed)
            assert abs(logp - np.log(np.exp(z[tok]) / np.exp(z).sum())) < 1e-12
            assert allowed is None or allowed[tok]
            n += 1
    assert n == 600


def test_restatement_known_cases():
    z = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    assert choose(z, 0.0, 1.0, 0, 1.0)[0] == 0 and choose(z, 0.1 - 1e-9, 1.0, 0, 1.0)[0] == 0  # F = .1 .5 .7 1
    assert choose(z, 0.1 + 1e-9, 1.0, 0, 1.0)[0] == 1
    assert choose(z, 0.69, 1.0, 0, 1.0)[0] == 2 and choose(z, 0.999, 1.0, 0, 1.0)[0] == 3
    assert choose(z, 0.9, 0.0, 0, 1.0)[0] == 1                                              # greedy ignores u
    assert choose(z, 0.99, 1.0, 2, 1.0)[0] == 3 and choose(z, 0.5, 1.0, 2, 1.0)[0] == 1     # top-2 = {1, 3}: F = 4/7, 1
    # top-p 0.5: ranks 1, 3, 2, 0 with masses before 0, .4, .7, .9 -> {1, 3} kept; after top-2 the same by renormalised mass
    assert choose(z, 0.99, 1.0, 0, 0.5)[0] == 3 and choose(z, 0.0, 1.0, 0, 0.5)[0] == 1
    assert choose(z, 0.99, 1.0, 0, 0.4 - 1e-9)[0] == 1                                      # the mass before rank 1 is .4
    assert choose(z, 0.99, 1.0, 0, 0.4 + 1e-9)[0] == 3
    assert choose(z, 0.99, 1.0, 0, 1.0, allowed=[1, 1, 1, 0])[0] == 2                       # F = 1/7, 5/7, 1 over {0, 1, 2}
    assert choose([1.0, 2.0, 2.0, 0.0], 0.3, 0.0, 0, 1.0)[0] == 1                           # lowest index among equals
    assert choose([1.0, 2.0, 2.0, 0.0], 0.9, 1.0, 1, 1.0)[0] == 1                           # rank by index among equals
    tok, logp, amb = choose(z, 0.5 + 1e-7, 1.0, 0, 1.0, eps=1e-5)
    assert tok == 2 and amb and abs(logp - np.log(0.2)) < 1e-12
    assert not choose(z, 0.45, 1.0, 0, 1.0, eps=1e-5)[2]


def test_check_against_oracle_with_an_allowed_mask():
    """check_against_oracle on sequences drawn by the rule itself from synthetic logits: with the `allowed` mask the
    sequences were drawn under, nothing disagrees and every unambiguous live decision is marked as checked; without it
    (the default), the rule would have drawn suppressed tokens and the sequences disagree; a wrong token is reported."""
    rs = np.random.RandomState(4)
    R, T, V, eos = 6, 40, 12, 1
    logits = rs.uniform(-2, 2, (R, T - 1, V))
    logits[:, :, eos] += 2.0                                  # '$' is likely: suppressing it changes the draws
    u = rs.rand(T, R)
    allowed = np.ones(V, np.uint8)
    allowed[[0, eos]] = 0
    for setting in ((1.0, 0, 1.0), (0.8, 5, 0.9)):
        tokens = np.zeros((R, T), np.int64)
        for r in range(R):
            for t in range(T - 1):
                tokens[r, t + 1] = choose(logits[r, t], u[t, r], *setting, allowed)[0]
        assert not np.isin(tokens[:, 1:], [0, eos]).any()
        res = check_against_oracle(tokens, u, logits, eos, *setting, allowed=allowed)
        assert not res["bad"] and res["live"] == R * (T - 1) and (res["lengths"] == T - 1).all()
        assert res["checked"].shape == (R, T) and not res["checked"][:, 0].any()
        assert int(res["checked"].sum()) == res["live"] - res["ambiguous"] and res["ambiguous"] <= 0.02 * res["live"]
        assert check_against_oracle(tokens, u, logits, eos, *setting)["bad"]
        wrong = tokens.copy()
        r, t = np.argwhere(res["checked"])[len(np.argwhere(res["checked"])) // 2]
        wrong[r, t] = 2 if wrong[r, t] != 2 else 3
        assert (int(r), int(t) - 1) in [b[:2] for b in check_against_oracle(wrong, u, logits, eos, *setting, allowed=allowed)["bad"]]


def test_sampling_refuses_cpu_tensors():
    import torch

    from singa_amd import ops
    from singa_amd.config import Config
    from singa_amd.model.Sampling import sample
    ex = Config()
    ex.protein_atom_feature = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        sample(None, ["&", "$", "^"], 2, 1, 8, ex, device="cpu")
    state = {"tokens": torch.zeros(2, 4, dtype=torch.int64), "next": torch.zeros(2, dtype=torch.int64),
             "finished": torch.zeros(2, dtype=torch.uint8), "length": torch.zeros(2, dtype=torch.int32),
             "sum_logp": torch.zeros(2), "live": torch.zeros(1, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_token(torch.zeros(2, 3), torch.zeros(4, 2), torch.zeros(1, dtype=torch.int64), 1, state)
