"""The device beam search, the part that runs without a GPU: the header against its binding table and the built library, the
argument errors of the entry points, the restatement of the rule (tests/beam_rule.py) against the package's own `_select` and
`BeamHypotheses` on whole searches without a mask, what the rule guarantees under each grammar, and gen.py's argument checks."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

from tests import beam_rule as BR
from tests import grammar_rule as G
from tests import valence_rule as VR
from tests.helpers import smi_voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_beam_expand", "singa_beam_select", "singa_beam_work"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_beam_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_beam.h"))))
    assert declared == sorted(_capi.BEAM_EXPORTS) == NAMES
    others = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS) | set(_capi.FORCE_EXPORTS) | \
        set(_capi.SWOR_EXPORTS) | set(_capi.STREAM_EXPORTS) | set(_capi.VALENCE_EXPORTS)
    assert not set(_capi.BEAM_EXPORTS) & others
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):                            # declared in its own header only
        if other != "singa_hip_beam.h":
            assert "singa_beam_" not in strip(other), other
    import __graft_entry__
    assert "singa_hip_beam.h" in open(__graft_entry__.__file__).read()                       # a dependency of the build


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    NULL, SHAPE = -1, -3
    err = lambda: lib.singa_last_error_string()

    def expand(rows=4, k=2, V=116, T=8, logits=p, cls=None, cap=None, gstate=None, vstate=None, cand=p, done=p):
        return lib.singa_beam_expand(logits, None, cls, cap, p, 1, rows, k, V, T, p, gstate, vstate, done, cand, None)

    def select(rows=4, k=2, V=116, T=8, eos=3, pad=4, cand=p, cls=None, cap=None, gstate=None, vstate=None, work=p, live=p, len_pow=p):
        return lib.singa_beam_select(cand, cls, cap, p, 1, rows, k, V, T, eos, pad, len_pow, p, p, p, p, p, gstate, vstate, p, p, p, p, p,
                                     p, p, p, live, work, None)

    for call in (expand, select):
        for null in (dict(cand=None), dict(cls=p), dict(gstate=p), dict(cls=p, gstate=p, vstate=p), dict(cls=p, gstate=p, cap=p),
                     dict(cap=p, vstate=p)):
            assert call(**null) == NULL, (call.__name__, null)
            assert b"beam_" in err()
        for bad in (dict(k=0), dict(k=1025, rows=1025), dict(rows=5), dict(rows=-2), dict(V=0), dict(V=1025), dict(T=1),
                    dict(T=2, cls=p, gstate=p), dict(T=2, cls=p, gstate=p, cap=p, vstate=p)):
            assert call(**bad) == SHAPE, (call.__name__, bad)
            assert b"beam_" in err()
        assert call(rows=0) == 0 and call(rows=0, k=1024, V=1024, T=2) == 0 and call(rows=0, T=3, cls=p, gstate=p) == 0
        assert call(rows=0, T=3, cls=p, gstate=p, cap=p, vstate=p) == 0
    assert expand(logits=None) == NULL and expand(done=None) == NULL
    assert select(work=None) == NULL and select(live=None) == NULL and select(len_pow=None) == NULL
    for bad in (dict(eos=116), dict(eos=-1), dict(pad=116), dict(pad=-1)):
        assert select(**bad) == SHAPE, bad
    assert select(work=ctypes.c_void_p(p.value + 4)) == SHAPE and b"aligned" in err()

    assert lib.singa_beam_work(-1, 8) == -1 and lib.singa_beam_work(4, 1) == -1 and lib.singa_beam_work(0, 2) == 0
    for rows, T in ((1, 2), (7, 41), (1024, 257)):                        # the new slots' columns and eight words each, aligned
        n = lib.singa_beam_work(rows, T)
        assert n % 16 == 0 and rows * (T * 8 + 32) <= n <= rows * (T * 8 + 32) + 9 * 16


# ------------------------------------------------------------------------------------------------ the restatement, pinned
def prefix_logits(prefix, pocket, V, eos, seed):
    """Logits that are a function of (pocket, prefix) alone, so that two searches that hold the same prefix in different rows
    see the same numbers; the '$' logit is pushed up or down by the prefix, so that it ranks inside and outside the first k."""
    key = zlib.crc32(np.asarray(prefix, np.int64).tobytes() + bytes([pocket, seed]))
    rs = np.random.RandomState(key)
    z = rs.randn(V).astype(np.float32)
    z[eos] += np.float32(rs.choice(([-3.0, -1.5, 0.0, 1.0], [-1.5, 0.0, 1.0, 2.5], [-1.5, 1.0, 2.5, 4.0])[seed % 3]))
    return z


def host_search(B, k, V, T, sos, eos, pad, seed):
    """`beam_search`'s loop around the package's `_select` and `BeamHypotheses`, fed with `prefix_logits`; the candidates are
    ranked as torch.topk would (the inputs have no ties).  -> (hyps, done step per pocket, the ranks '$' was seen at)"""
    from singa_amd.model.BeamSearch import BeamHypotheses, _select
    rows = B * k
    scores = np.zeros((B, k), np.float32)
    scores[:, 1:] = -1e9
    scores = scores.reshape(-1)
    prefixes = np.full((rows, 1), sos, np.int64)
    done, done_step = [False] * B, [None] * B
    hyps = [BeamHypotheses(k, T, length_penalty=0.7) for _ in range(B)]
    eos_ranks = []
    cur_len = 1
    while cur_len < T:
        lp = BR.log_probs(np.stack([prefix_logits(prefixes[r], r // k, V, eos, seed) for r in range(rows)]))
        cand = (lp + scores[:, None]).astype(np.float32).reshape(B, k * V)
        flat = np.argsort(-cand.astype(np.float64), axis=1, kind="stable")[:, :2 * k]
        value = np.take_along_axis(cand, flat, 1)
        live = [b for b in range(B) if not done[b]]                           # (a done pocket's rows are all alike)
        assert (np.diff(value[live].astype(np.float64), axis=1) < 0).all()    # no ties: the rank is the host rule's own
        eos_ranks += [r for b in range(B) if not done[b] for r in range(2 * k) if flat[b, r] % V == eos]
        before = list(done)
        s, tk, src = _select(value, flat, prefixes, hyps, done, k, V, eos, pad, cur_len)
        for b in range(B):
            if done[b] and not before[b]:
                done_step[b] = cur_len - 1
        if all(done):
            break
        scores = s
        prefixes = np.concatenate([prefixes[src], tk[:, None]], axis=1)
        cur_len += 1
    final = [h.beams[:] for h in hyps]
    for b in range(B):
        if not done[b]:
            for j in range(k):
                hyps[b].add(prefixes[b * k + j], float(scores[b * k + j]))
    return final, hyps, done_step, eos_ranks


@pytest.mark.parametrize("k", [1, 3, 5])
def test_rule_without_mask_is_the_host_selection(k):
    B, V, T = 2, 116, 12
    sos, eos, pad = 0, 1, 2
    seen_done, seen_in, seen_out, seen_full, seen_open, seen_drop = 0, 0, 0, 0, 0, 0
    for seed in range(9):
        stored, hyps, done_step, eos_ranks = host_search(B, k, V, T, sos, eos, pad, seed)
        run = BR.Search(B, k, V, T, sos, eos, pad)
        for t in range(T - 1):
            if run.done.all():
                break
            logits = np.stack([prefix_logits(run.tokens[b, i, :t + 1], b, V, eos, seed) for b in range(B) for i in range(k)])
            run.step(logits)
        assert run.done_step == done_step, seed
        for stage, want in (("before", stored), ("after", [h.beams for h in hyps])):     # in front of and behind BS:141-149
            for b in range(B):
                got = run.hyps[b].items
                assert [it[0] for it in got] == [s for s, _ in want[b]], (seed, stage, b)      # same doubles, same order
                assert all(np.array_equal(it[2], x) for it, (_, x) in zip(got, want[b])), (seed, stage, b)
            if stage == "before":
                run.finish()
        assert [h.worst for h in run.hyps] == [h.worst_score for h in hyps]
        seen_done += sum(d is not None for d in done_step)
        seen_in += sum(r < k for r in eos_ranks)
        seen_out += sum(r >= k for r in eos_ranks)
        seen_full += sum(len(h.beams) == k for h in hyps)
        seen_open += sum(d is None for d in done_step)
        seen_drop += sum(h.dropped for h in run.hyps)
    print(f"k = {k}: {seen_done} pockets done early, {seen_open} not; '$' ranked inside the first k {seen_in} times, outside "
          f"{seen_out} times; {seen_drop} stored hypotheses dropped for a better one")
    assert seen_done > 0 and seen_open > 0 and seen_in > 0 and seen_out > 0 and seen_full > 0 and (seen_drop > 0 or k == 1)


# ------------------------------------------------------------------------------------------------ what the rule guarantees
@pytest.mark.parametrize("T", [3, 4, 12])
@pytest.mark.parametrize("grammar", ["smiles", "valence"])
def test_rule_under_a_grammar_stores_only_strings_that_parse(grammar, T):
    from singa_amd import smiles
    voc = [str(v) for v in smi_voc()]
    V, sos, eos, pad = len(voc), voc.index("&"), voc.index("$"), voc.index("^")
    cap = smiles.capacity(voc)
    capacity = {t: int(c) for t, c in zip(voc, cap)}
    cls = smiles.classify_orders(voc) if grammar == "valence" else smiles.classify(voc)
    structure = [i for i, t in enumerate(voc) if t in "()=#123"]
    died = 0
    for k in (1, 3, 5):
        rs = np.random.RandomState(100 * T + k)
        run = BR.Search(2, k, V, T, sos, eos, pad, cls=cls, cap=cap if grammar == "valence" else None)
        for t in range(T - 1):
            z = rs.randn(2 * k, V).astype(np.float32)
            z[:, structure] += 3.0                                             # branches, rings and multiple bonds are common
            z[:, eos] += rs.choice([-2.0, 3.0], size=2 * k)
            run.step(z)
            died += int((run.score[~run.done] == BR.NEG).sum())
        assert not (run.live > 0).any()                                        # no live beam is left to be added unfinished
        run.finish()
        for b in range(2):
            assert len(run.hyps[b].items) >= 1
            for score, total, toks, stamp in run.hyps[b].items:
                assert stamp >= 0 and len(toks) <= T - 1
                text = [voc[x] for x in toks[1:]]
                assert G.parses(text), "".join(text)
                if grammar == "valence":
                    assert not VR.over_capacity(text, capacity), "".join(text)
    if T <= 4:
        assert died > 0                                                        # the budget leaves slots without a candidate


def test_gen_accepts_a_grammar_under_beam_search():
    import gen
    for grammar in ("smiles", "valence"):
        args = gen.parse_args(["--mode", "beam", "--grammar", grammar])
        assert args.mode == "beam" and args.grammar == grammar and args.beam_select == "host"
    assert gen.parse_args(["--mode", "beam", "--beam-select", "device"]).beam_select == "device"
    assert gen.parse_args(["--mode", "beam"]).grammar == "none"
    with pytest.raises(AssertionError, match="beam mode only"):
        gen.parse_args(["--mode", "sample", "--beam-select", "device"])
    with pytest.raises(AssertionError, match="valence"):
        gen.parse_args(["--mode", "distinct", "--grammar", "valence"])
    assert "beam_search_device" in gen.__doc__ and "beam search is not constrained" not in gen.__doc__
