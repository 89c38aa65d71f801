"""Lab: cut the golden 3-graph step at the embedding / transformer boundary (SINGA.forward(boundary=...)), record the two
embedding outputs, the gradients the transformer returns for them and every PoswiseFeedForward ReLU mask -> .pt.  With a
third argument the embedding outputs are REPLACED by the ones of that earlier dump, so that two library builds can be run on
bit-identical transformer inputs."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from singa_amd import _lib
if os.environ.get("SINGA_PROBE_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["SINGA_PROBE_LIB"])
from singa_amd import ops
from tests.helpers import NAMES, golden, product_batch, state_from_spec
from singa_amd.config import load_config
from singa_amd.model.GAN import SINGA
L = int(sys.argv[1])
masks = []
_fwd = ops._PosFFN.forward


def fwd(ctx, *args):
    y = _fwd(ctx, *args)
    masks.append((ctx.to_save[3] > 0).cpu())
    return y


ops._PosFFN.forward = staticmethod(fwd)
sd = state_from_spec(f"singa_L{L}")
z = golden(f"singa_L{L}_B3.npz")
model = SINGA(load_config(lmax=L), device="cuda")
model.load_state_dict(sd, strict=False)
model.eval()
g = product_batch(NAMES, z)
boundary = []
if len(sys.argv) > 3:
    other = torch.load(sys.argv[3])
    _detach = torch.Tensor.detach
    from singa_amd.model import GAN as _G
    _emb_call = model.embedding.forward
    from singa_amd.graph import PA, LA

    def emb(gg):
        out = _emb_call(gg)
        with torch.no_grad():
            out[PA].embedding.copy_(other["xa"].cuda())
            out[LA].embedding.copy_(other["xl"].cuda())
        return out

    model.embedding.forward = emb
logits = model(g, boundary=boundary)
loss = torch.nn.functional.cross_entropy(logits, g["ligand_data"]["smiIndices_tgt"].reshape(-1))
loss.backward()
torch.cuda.synchronize()
(xa, da), (xl, dl) = boundary
torch.save({"xa": xa.detach().cpu(), "xl": xl.detach().cpu(), "ga": da.grad.cpu(), "gl": dl.grad.cpu(), "masks": masks,
            "loss": float(loss)}, sys.argv[2])
