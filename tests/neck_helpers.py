"""Shared by tests/test_neck.py (CPU) and tests/test_neck_kernels.py (GPU): the reference fixture of the RPN neck
(tests/golden/neck_golden.npz, written by tests/golden/make_neck_golden.py) and float64 references of single layers."""
import copy
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neck_golden.npz")
C3S1, C3S2, C1, D2 = 0, 1, 2, 3
KIND_NAMES = {C3S1: "C3S1", C3S2: "C3S2", C1: "C1", D2: "D2"}
E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5  # include/shasta_hip.h
SHIPPED = dict(layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
               us_num_filters=[256, 256], num_input_features=256)  # the neck block of configs/nusc/*.py


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    cfg = {k[4:]: z[k].tolist() for k in z.files if k.startswith("cfg_")}
    keys = z["keys"].tolist()
    init = {k: z["init/" + k] for k in keys}
    used = {k: z["used/" + k] if "used/" + k in z.files else init[k] for k in keys}
    return dict(seed=int(z["seed"]), cfg=cfg, keys=keys, init=init, used=used, x=z["x"], y32=z["y32"], y64=z["y64"])


def build_fixture_neck(load_used=True):
    """The fixture's config through the registry under the fixture's seed; with the as-used tensors loaded, in eval mode."""
    from shasta_amd import builder
    fx = fixture()
    torch.manual_seed(fx["seed"])
    m = builder.build_neck(dict(type="RPN", **fx["cfg"]))
    if load_used:
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["used"].items()})
    return m.eval()


def randomize_bn(module, gen):
    """Non-trivial BatchNorm weight, bias and running statistics from a seeded generator."""
    with torch.no_grad():
        for mod in module.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(0.5 + torch.rand(n, generator=gen))
                mod.bias.copy_(0.1 * torch.randn(n, generator=gen))
                mod.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=gen))


def layers64(module, x):
    """forward_layers of a float64 copy of `module` on the CPU, eval mode."""
    m64 = copy.deepcopy(module).cpu().double().eval()
    with torch.no_grad():
        return m64.forward_layers(x.detach().cpu().double())


def layer_tensors(kind, cin, cout, gen):
    """Weight in the layer's own layout (K0-sized values: products sum to O(1)) and random BatchNorm tensors [gamma, beta, mean, var]."""
    taps = 9 if kind in (C3S1, C3S2) else 1
    shape = (cout, cin, 3, 3) if taps == 9 else (cin, cout, 1, 1) if kind == C1 else (cin, cout, 2, 2)
    w = torch.randn(shape, generator=gen) / float(np.sqrt(cin * taps))
    bn = [0.5 + torch.rand(cout, generator=gen), 0.2 * torch.randn(cout, generator=gen), 0.3 * torch.randn(cout, generator=gen),
          0.5 + torch.rand(cout, generator=gen)]
    return w, bn


def layer_ref64(kind, x, w, bn, eps):
    """torch's CPU float64 conv2d / conv_transpose2d + eval batch_norm + ReLU."""
    x, w = x.double(), w.double()
    if kind == C3S1:
        y = F.conv2d(x, w, padding=1)
    elif kind == C3S2:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1)), w, stride=2)
    elif kind == C1:
        y = F.conv_transpose2d(x, w, stride=1)
    else:
        y = F.conv_transpose2d(x, w, stride=2)
    g, b, mean, var = [t.double() for t in bn]
    return F.relu(F.batch_norm(y, mean, var, g, b, training=False, eps=eps))
