"""YAML -> attribute-dict configuration (what the reference gets from EasyDict, utils/misc.py:137-146)."""
import copy
import os

import yaml

DEFAULT_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "train.yml")


class Config(dict):
    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = v

    def __setitem__(self, k, v):
        super().__setitem__(k, Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def to_dict(self):
        """Plain nested dicts/lists (what a checkpoint stores, so that `torch.load(weights_only=True)` accepts it)."""
        def plain(v):
            if isinstance(v, dict):
                return {k: plain(x) for k, x in v.items()}
            return [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
        return plain(self)

    def __deepcopy__(self, memo):
        return Config({k: copy.deepcopy(v, memo) for k, v in self.items()})


SUPPORTED_LMAX = (2, 3, 4, 6)
SUPPORTED_MMAX = 2


def validate_embedding_config(emb):
    """Refuses, before anything is launched and without a GPU, every `embedding` section that the HIP launchers would refuse
    at their first call with SINGA_E_LMAX / SINGA_E_SHAPE.  `emb`: the `embedding` section (attribute access).  Raises
    ValueError naming the YAML key; returns (lmax, mmax) of the one resolution.

    Built: one resolution, lmax 2, 3, 4 or 6 at mmax = 2 (the edge S2 kernels and the three-segment SO(2) convolution layout are
    written for m <= 2), 16 sphere channels (gather-rotate, rmsnorm, the skinny SO(3) linears), 128 hidden attention channels
    (the edge S2 grid), 7 heads of 16 value channels (rotate-back-scatter), no dropout, the shared atom-edge embedding.
    `ffn_hidden_channels` is not checked here: the default path constructs at any width and `recompute=True` refuses all but
    512 itself (FeedForwardNetwork)."""
    def bad(key, got, want):
        raise ValueError(f"embedding.{key} = {got!r}: the HIP kernels are built for {want}")

    lmax_list, mmax_list = list(emb.lmax_list), list(emb.mmax_list)
    if len(lmax_list) != 1:
        bad("lmax_list", lmax_list, "one resolution (a list of one degree)")
    if len(mmax_list) != 1:
        bad("mmax_list", mmax_list, "one resolution (a list of one order)")
    lmax, mmax = lmax_list[0], mmax_list[0]
    if isinstance(lmax, bool) or int(lmax) != lmax or int(lmax) not in SUPPORTED_LMAX:
        bad("lmax_list", lmax_list, "lmax 2, 3, 4 or 6")
    if isinstance(mmax, bool) or int(mmax) != mmax or int(mmax) != SUPPORTED_MMAX:
        bad("mmax_list", mmax_list, "mmax 2")
    if int(emb.sphere_channels) != 16:
        bad("sphere_channels", emb.sphere_channels, "16 sphere channels")
    if int(emb.attn_hidden_channels) != 128:
        bad("attn_hidden_channels", emb.attn_hidden_channels, "128 hidden attention channels")
    if int(emb.num_heads) != 7:
        bad("num_heads", emb.num_heads, "7 heads")
    if int(emb.attn_value_channels) != 16:
        bad("attn_value_channels", emb.attn_value_channels, "16 value channels per head")
    if not (emb.share_atom_edge_embedding and emb.use_atom_edge_embedding):
        bad("share_atom_edge_embedding / embedding.use_atom_edge_embedding",
            (emb.share_atom_edge_embedding, emb.use_atom_edge_embedding), "the shared atom-edge embedding (both true)")
    for key in ("alpha_drop", "proj_drop", "drop_path_rate"):
        if float(getattr(emb, key)) != 0.0:
            bad(key, getattr(emb, key), "0.0 (no dropout)")
    return int(lmax), int(mmax)


def load_config(path=None, lmax=None):
    with open(path or DEFAULT_PATH) as f:
        cfg = Config(yaml.safe_load(f))
    if lmax is not None:
        cfg.embedding.lmax_list = [int(lmax)]
    L = int(cfg.embedding.lmax_list[0])
    cfg.model.featurizer_feat_dim = (L + 1) ** 2 * int(cfg.embedding.sphere_channels)
    return cfg
