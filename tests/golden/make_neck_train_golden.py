"""Generates tests/golden/neck_train_golden.npz from the REFERENCE's RPN neck (det3d/models/necks/rpn.py, imported in place through
ref_import; fixture generation only - it runs where the reference exists) in train() mode, as the reference's training step runs the
frozen neck (tools/nusc_shasta/train.py:184-193): every BatchNorm2d on batch statistics, every one updating its running statistics.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_neck_train_golden.py

The config and the seed of make_neck_golden.py; the file holds
    seed, cfg_* (the config as plain numbers), keys (the state_dict key list, in order),
    used/<key>   every tensor as used in the forward WHERE IT DIFFERS from the tensor as first constructed, which neck_golden.npz holds
                 as init/<key> (BatchNorm weight, bias and running statistics from a seeded generator; the running means are kept away
                 from zero - 0.3 .. 0.8 in magnitude - so that a relative bar on the updated ones means something),
    x            randn(2, 16, 10, 38) + 0.25 (the backbone's output is not clipped: both signs),
    y32, y64     the reference's CPU forward in train() mode: fp32, and the same module (same starting state) after .double(),
    after/<key>  running_mean, running_var (float64) and num_batches_tracked of every BatchNorm2d after the float64 forward.
"""
import copy
import importlib
import logging
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

SEED = 20
CFG = dict(layer_nums=[2, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
           num_input_features=16)


def main():
    ref_import.import_shasta()  # installs the stubs and the reference on sys.path
    R = importlib.import_module("det3d.models.necks.rpn")
    torch.manual_seed(SEED)
    m = R.RPN(logger=logging.getLogger("make_neck_train_golden"), **CFG).train()
    keys = list(m.state_dict().keys())
    out = {"seed": np.int64(SEED), "keys": np.array(keys)}
    for k, v in CFG.items():
        out["cfg_" + k] = np.asarray(v, np.int64)
    init = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}  # = init/<key> of neck_golden.npz: same seed, same config
    g = torch.Generator().manual_seed(SEED + 2)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(0.5 + torch.rand(n, generator=g))
                mod.bias.copy_(0.1 * torch.randn(n, generator=g))
                sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
                mod.running_mean.copy_(sign * (0.3 + 0.5 * torch.rand(n, generator=g)))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
    for k, v in m.state_dict().items():
        if not np.array_equal(v.numpy(), init[k]):
            out["used/" + k] = v.detach().clone().numpy()
    x = torch.randn(2, 16, 10, 38, generator=g) + 0.25
    m64 = copy.deepcopy(m).double()
    assert m.training and m64.training
    with torch.no_grad():
        y32 = m(x)
        y64 = m64(x.double())
    nbn = 0
    for k, v in m64.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["after/" + k] = v.detach().clone().numpy()
            nbn += k.endswith("running_mean")
    out.update(x=x.numpy(), y32=y32.numpy(), y64=y64.numpy())
    path = os.path.join(HERE, "neck_train_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d keys, %d BatchNorm2d modules, output %s, max|y32 - y64| = %.3e, %d bytes"
          % (path, len(keys), nbn, tuple(y32.shape), float(np.abs(y32.numpy() - y64.numpy()).max()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
