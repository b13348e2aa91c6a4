"""Generates tests/golden/neck_golden.npz from the REFERENCE's RPN neck (det3d/models/necks/rpn.py, imported in place through
ref_import; fixture generation only - it runs where the reference exists).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_neck_golden.py

A small neck with every layer kind of the shipped configs (stride-1 and stride-2 blocks, the 1x1 and the 2x2 stride-2 deblock) is
built under torch.manual_seed(seed); the file holds
    seed, cfg_* (the config as plain numbers), keys (the state_dict key list, in order),
    init/<key>   every tensor as first constructed (pins module creation order = RNG order),
    used/<key>   every tensor as used in the forward WHERE IT DIFFERS from init/<key> (the BatchNorm weight, bias, running_mean and
                 running_var get non-trivial values from a seeded generator; the convolution weights are used as constructed),
    x            relu(randn(2, 16, 10, 38)),
    y32, y64     the reference's CPU forward in eval mode: fp32, and the same module after .double().
"""
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
    m = R.RPN(logger=logging.getLogger("make_neck_golden"), **CFG).eval()
    keys = list(m.state_dict().keys())
    out = {"seed": np.int64(SEED), "keys": np.array(keys)}
    for k, v in CFG.items():
        out["cfg_" + k] = np.asarray(v, np.int64)
    init = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}
    for k, v in init.items():
        out["init/" + k] = v
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(0.5 + torch.rand(n, generator=g))
                mod.bias.copy_(0.1 * torch.randn(n, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
    nused = 0
    for k, v in m.state_dict().items():
        if not np.array_equal(v.numpy(), init[k]):
            out["used/" + k] = v.detach().clone().numpy()
            nused += 1
    x = torch.relu(torch.randn(2, 16, 10, 38, generator=g))
    with torch.no_grad():
        y32 = m(x)
        y64 = m.double()(x.double())
    out.update(x=x.numpy(), y32=y32.numpy(), y64=y64.numpy())
    path = os.path.join(HERE, "neck_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d keys (%d values, %d changed for the forward), output %s, max|y32 - y64| = %.3e, %d bytes"
          % (path, len(keys), sum(v.size for v in init.values()), nused, tuple(y32.shape),
             float(np.abs(y32.numpy() - y64.numpy()).max()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
