"""What the ancestry-indexed cache path (include/singa_hip_ancestry.h) refuses before anything is launched: no GPU needed."""
import pytest
import torch


def test_refusals_before_any_launch():
    import gen
    from singa_amd import ops
    from singa_amd.model.BeamSearch import beam_search_device
    from singa_amd.model.Sampling import sample_distinct
    for fn in (sample_distinct, beam_search_device):
        with pytest.raises(ValueError, match="cache is 'copy' or 'ancestry'"):
            fn(None, None, 2, 1, 8, *([1] if fn is beam_search_device else []), None, cache="moved")
    x = torch.zeros(2, 256)
    with pytest.raises(ValueError, match="per_row"):
        ops.dec_layer_step(x, None, None, None, torch.zeros(2, dtype=torch.int64), None, None, None, 1, per_row=True,
                           anc=torch.zeros(4, 2, dtype=torch.int32))
    for argv in (["--mode", "sample", "--kv-cache", "ancestry"], ["--mode", "beam", "--kv-cache", "copy"],
                 ["--mode", "score", "--molecules", "f.tsv", "--kv-cache", "ancestry"]):
        with pytest.raises(SystemExit):
            gen.parse_args(argv)
    assert gen.parse_args(["--mode", "distinct", "--kv-cache", "ancestry"]).kv_cache == "ancestry"
    assert gen.parse_args(["--mode", "beam", "--beam-select", "device", "--kv-cache", "ancestry"]).kv_cache == "ancestry"
    assert gen.parse_args(["--mode", "distinct"]).kv_cache == "copy"
