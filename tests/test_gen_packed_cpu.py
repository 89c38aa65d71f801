"""Generation over a packed dataset, the host side (singa_amd/generate.py, gen.py's argument checks): the split's ids and
their passes, the per-pocket uniforms and what they depend on, and every combination of flags gen.py accepts or refuses
before a device is touched.  No GPU."""
import numpy as np
import pytest
import torch

from singa_amd import dataset as D
from singa_amd import graph as G

PACKED = ["--data", "packed", "--dataset", "D"]


# ---------------------------------------------------------------------------------------------------------------- gen.py
@pytest.mark.parametrize("mode", [["--mode", "sample"], ["--mode", "distinct"], ["--mode", "beam"],
                                  ["--mode", "score", "--molecules", "dataset"]], ids=lambda m: m[1])
def test_gen_accepts_a_pack_in_every_mode(mode):
    import gen
    a = gen.parse_args(PACKED + mode)
    assert a.data == "packed" and a.dataset == "D" and a.split == "test" and a.first is None and not a.prop_from_dataset
    assert a.mode == mode[1]
    if a.mode == "score":
        assert a.molecules == "dataset"
    a = gen.parse_args(PACKED + mode + ["--split", "val", "--first", "3", "--pockets-per-pass", "2", "--prop-from-dataset"])
    assert (a.split, a.first, a.pockets_per_pass, a.prop_from_dataset) == ("val", 3, 2, True)


@pytest.mark.parametrize("argv,want", [
    (["--mode", "sample", "--num-samples", "100"], 20), (["--mode", "sample", "--num-samples", "2048"], 1),
    (["--mode", "distinct", "--num-samples", "5000"], 1), (["--mode", "beam", "--num-beams", "20"], 102),
    (["--mode", "sample", "--num-samples", "5000", "--rows-per-pocket", "64"], 32),
    (["--mode", "score", "--molecules", "dataset", "--rows-per-pocket", "256"], 8)])
def test_gen_default_pockets_per_pass(argv, want):
    """The largest P with P x rows per pocket <= 2048, at least 1; rows per pocket: --rows-per-pocket, else --num-samples or
    --num-beams."""
    import gen
    assert gen.parse_args(PACKED + argv).pockets_per_pass == want


@pytest.mark.parametrize("argv", [
    ["--data", "packed"],                                                      # no --dataset
    ["--dataset", "D"], ["--split", "test"], ["--first", "2"], ["--pockets-per-pass", "2"], ["--prop-from-dataset"],
    ["--mode", "score", "--molecules", "dataset"],                             # each of them without --data packed
    ["--data", "synthetic", "--dataset", "D"],
    PACKED + ["--pockets", "3"],
    PACKED + ["--first", "0"], PACKED + ["--first", "-2"],
    PACKED + ["--pockets-per-pass", "0"], PACKED + ["--pockets-per-pass", "-1"]], ids=lambda a: " ".join(a))
def test_gen_refuses(argv):
    import gen
    with pytest.raises(SystemExit):
        gen.parse_args(argv)


def test_gen_parses_the_earlier_argument_vectors_as_before():
    """The vectors of tests/test_prefix_cpu.py and tests/test_beam_device_cpu.py: same outcome, and none of them has become a
    packed run."""
    import gen
    for argv, check in (
            (["--mode", "distinct", "--prefix", "c1ccc(", "--grammar", "smiles"], lambda a: a.prefix == "c1ccc(" and a.mode == "distinct"),
            (["--mode", "beam", "--beam-select", "device", "--prefix", "CC"], lambda a: a.prefix == "CC" and a.beam_select == "device"),
            (["--mode", "beam", "--grammar", "valence", "--prefix", "CC"], lambda a: a.prefix == "CC"),
            (["--mode", "sample", "--rows-per-pocket", "8", "--prefix", "CC"], lambda a: a.rows_per_pocket == 8 and a.prefix == "CC"),
            (["--mode", "score", "--molecules", "x.tsv", "--rows-per-pocket", "4"], lambda a: a.rows_per_pocket == 4 and a.molecules == "x.tsv"),
            (["--mode", "beam", "--grammar", "smiles"], lambda a: a.grammar == "smiles" and a.beam_select == "host"),
            (["--mode", "beam", "--grammar", "valence"], lambda a: a.grammar == "valence" and a.beam_select == "host"),
            (["--mode", "beam", "--beam-select", "device"], lambda a: a.beam_select == "device"),
            (["--mode", "beam"], lambda a: a.grammar == "none")):
        a = gen.parse_args(argv)
        assert check(a), argv
        assert a.data == "golden" and a.pockets == 3 and a.dataset is None and a.pockets_per_pass is None and a.first is None
    for argv in (["--mode", "beam", "--prefix", "CC"], ["--mode", "score", "--molecules", "x.tsv", "--prefix", "CC"],
                 ["--mode", "distinct", "--rows-per-pocket", "4"], ["--mode", "beam", "--rows-per-pocket", "4"]):
        with pytest.raises(SystemExit):
            gen.parse_args(argv)
    with pytest.raises(AssertionError, match="beam mode only"):
        gen.parse_args(["--mode", "sample", "--beam-select", "device"])
    with pytest.raises(AssertionError, match="valence"):
        gen.parse_args(["--mode", "distinct", "--grammar", "valence"])
    assert gen.parse_args(["--data", "synthetic", "--pockets", "5"]).pockets == 5
    for word in ("--data packed", "--pockets-per-pass", "singa_amd/generate.py"):
        assert word in gen.__doc__


# ---------------------------------------------------------------------------------------------------------------- passes
@pytest.mark.parametrize("P,sizes", [(1, [1] * 7), (2, [2, 2, 2, 1]), (3, [3, 3, 1]), (7, [7]), (9, [7])])
def test_passes(P, sizes):
    from singa_amd.generate import passes
    ids = np.array([12, 3, 5, 40, 41, 0, 9], np.int64)
    chunks = passes(ids, P)
    assert [len(c) for c in chunks] == sizes
    assert np.array_equal(np.concatenate(chunks), ids)
    with pytest.raises(ValueError, match="pockets_per_pass"):
        passes(ids, 0)


# ---------------------------------------------------------------------------------------------------------------- split_ids
def test_split_ids():
    from singa_amd.generate import split_ids
    gs = [G.synthetic_graph(i, n_protein=20, n_ligand=5, e_pp=40, e_ll=8, e_x=6, tgt_len=64, with_lap=False) for i in range(6)]
    pack = D.PackedDataset.from_graphs(gs, names=[f"g{i}" for i in range(6)], splits={"train": [4, 0, 2], "test": [5, 1, 3], "val": []})
    got = split_ids(pack, "test")
    assert got.dtype == np.int64 and got.tolist() == [5, 1, 3]                 # stored order, not sorted
    assert split_ids(pack, "train").tolist() == [4, 0, 2]
    assert split_ids(pack, "test", first=2).tolist() == [5, 1]
    assert split_ids(pack, "test", first=10).tolist() == [5, 1, 3]
    for missing in ("val", "holdout"):                                         # empty, absent
        with pytest.raises(ValueError) as e:
            split_ids(pack, missing)
        assert "train" in str(e.value) and "test" in str(e.value) and missing in str(e.value)
    with pytest.raises(ValueError, match="first"):
        split_ids(pack, "test", first=0)


# ---------------------------------------------------------------------------------------------------------------- uniforms
def test_pocket_uniforms():
    from singa_amd.generate import pocket_seed, pocket_uniforms
    T, per = 16, 4
    alone = pocket_uniforms(1, [5], per, T, "cpu")
    assert alone.shape == (T, per) and alone.dtype == torch.float32
    assert float(alone.min()) >= 0.0 and float(alone.max()) < 1.0
    a, b = pocket_uniforms(1, [5, 7], per, T, "cpu"), pocket_uniforms(1, [2, 5], per, T, "cpu")
    assert a.shape == (T, 2 * per) and b.shape == (T, 2 * per)
    # pocket-major: the columns of graph 5 are the first `per` of [5, 7] and the last `per` of [2, 5], and are its own
    assert torch.equal(a[:, :per], alone) and torch.equal(b[:, per:], alone)
    assert torch.equal(pocket_uniforms(1, [5], per, T, "cpu"), alone)          # across two calls
    assert torch.equal(a[:, per:], pocket_uniforms(1, [7], per, T, "cpu"))
    assert not torch.equal(pocket_uniforms(2, [5], per, T, "cpu"), alone)      # another seed
    assert not torch.equal(a[:, per:], alone) and not torch.equal(b[:, :per], alone)   # another id
    assert len({pocket_seed(s, g) for s in range(8) for g in range(64)}) == 512
    assert all(0 <= pocket_seed(s, g) < 2 ** 63 for s in (0, -1, 2 ** 64 + 3) for g in (0, 2 ** 40))
