"""nn.Linear with the library's GEMM-only backward (ops.linear): same parameters, same state-dict keys."""
import torch.nn as nn

from . import ops


class Linear(nn.Linear):
    precision = "f32"        # of its GEMMs (ops.linear); model.CProMG.set_precision switches the transformer's Linears

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias, self.precision)
