"""Shared by tests/test_backbone.py (CPU) and tests/test_backbone_kernels.py (GPU): references of the sparse backbone that need neither
spconv nor a GPU.

  * the DENSE RESTATEMENT: a sparse tensor is a dense (B, C, D, H, W) tensor with exact zeros at inactive sites plus a (B, 1, D, H, W)
    mask.  A submanifold convolution is conv3d(padding 1) times the mask; a sparse convolution is conv3d(stride, padding) at the sites
    where max_pool3d(mask, k, s, p) > 0.  Any dtype (float64: the reference of the GPU tests; float32: its own error against float64 sets
    their bar).
  * a brute-force per-site Python loop over one convolution, used only to check the restatement itself.
  * numpy brute force of the index kernels: output coordinates (sorted by linear index) and neighbour tables.
  * a clustered-voxel generator: Gaussian blobs plus voxels on corners and faces of the grid.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5  # include/shasta_hip.h
SUBM = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
GEOMETRIES = {  # name -> (kernel, stride, padding), the four of SpMiddleResNetFHD
    "subm": SUBM,
    "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
    "k3s2p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1)),
    "k311s211p0": ((3, 1, 1), (2, 1, 1), (0, 0, 0)),
}


def out_grid(grid, geom):
    k, s, p = geom
    return tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(grid, k, s, p))


# ---- voxels -------------------------------------------------------------------------------------------------------
def clustered_voxels(rng, B, grid, blobs=3, per_blob=100, sigma=(2.0, 4.0, 4.0), empty_items=(), edges=True):
    """(V, 4) int32 unique (b, z, y, x) rows in a shuffled order: `blobs` Gaussian blobs per batch item, plus (edges) the eight corners
    and the six face centres of the grid in item 0 - the same (z, y, x) in two items where both have them.  Items in `empty_items` get
    no voxel."""
    D, H, W = grid
    rows = set()
    for b in range(B):
        if b in empty_items:
            continue
        for _ in range(blobs):
            c = rng.uniform([0, 0, 0], [D, H, W])
            pts = np.floor(c + rng.normal(size=(per_blob, 3)) * np.asarray(sigma)).astype(np.int64)
            ok = np.all((pts >= 0) & (pts < [D, H, W]), axis=1)
            rows.update((b, int(z), int(y), int(x)) for z, y, x in pts[ok])
        if edges:
            for z, y, x in itertools.product((0, D - 1), (0, H - 1), (0, W - 1)):
                rows.add((b, z, y, x))
            if b == 0:
                for z, y, x in ((0, H // 2, W // 2), (D - 1, H // 2, W // 2), (D // 2, 0, W // 2), (D // 2, H - 1, W // 2),
                                (D // 2, H // 2, 0), (D // 2, H // 2, W - 1)):
                    rows.add((b, z, y, x))
    out = np.array(sorted(rows), np.int32).reshape(-1, 4)
    return out[rng.permutation(len(out))]


def random_voxels(rng, B, grid, n):
    """Exactly n unique rows, uniform over the grid (n <= cells)."""
    D, H, W = grid
    lin = rng.choice(B * D * H * W, size=n, replace=False)
    out = np.stack([lin // (D * H * W), lin // (H * W) % D, lin // W % H, lin % W], axis=1).astype(np.int32)
    return out


# ---- numpy brute force of the index kernels -----------------------------------------------------------------------
def out_coords_ref(coords, B, grid, geom):
    """Active output sites of a sparse convolution, sorted by linear index ((b D + z) H + y) W + x: (n_out, 4) int32."""
    k, s, p = geom
    Do, Ho, Wo = out_grid(grid, geom)
    found = set()
    for b, z, y, x in coords.tolist():
        for tz, ty, tx in itertools.product(range(k[0]), range(k[1]), range(k[2])):
            nz, ny, nx = z + p[0] - tz, y + p[1] - ty, x + p[2] - tx
            if nz < 0 or ny < 0 or nx < 0 or nz % s[0] or ny % s[1] or nx % s[2]:
                continue
            oz, oy, ox = nz // s[0], ny // s[1], nx // s[2]
            if oz < Do and oy < Ho and ox < Wo:
                found.add((b, oz, oy, ox))
    return np.array(sorted(found), np.int32).reshape(-1, 4)


def neighbors_ref(out_coords, in_coords, grid, geom):
    """(n_out, K) int32: the input row at o * s - p + t, -1 where absent; `grid` is the INPUT level's."""
    k, s, p = geom
    row = {tuple(c): i for i, c in enumerate(in_coords.tolist())}
    taps = list(itertools.product(range(k[0]), range(k[1]), range(k[2])))
    nbr = np.full((len(out_coords), len(taps)), -1, np.int32)
    for o, (b, oz, oy, ox) in enumerate(out_coords.tolist()):
        for t, (tz, ty, tx) in enumerate(taps):
            z, y, x = oz * s[0] - p[0] + tz, oy * s[1] - p[1] + ty, ox * s[2] - p[2] + tx
            if 0 <= z < grid[0] and 0 <= y < grid[1] and 0 <= x < grid[2]:
                nbr[o, t] = row.get((b, z, y, x), -1)
    return nbr


# ---- the dense restatement ----------------------------------------------------------------------------------------
def to_dense(features, coords, B, grid):
    """(x, mask): (B, C, D, H, W) with zeros at inactive sites, (B, 1, D, H, W) of 0 / 1, both of features' dtype."""
    c = torch.as_tensor(coords).long()
    x = torch.zeros(B, features.shape[1], *grid, dtype=features.dtype)
    mask = torch.zeros(B, 1, *grid, dtype=features.dtype)
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = features
    mask[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1
    return x, mask


def rows_of(x, coords):
    """The (n, C) rows of a dense (B, C, D, H, W) tensor at `coords`."""
    c = torch.as_tensor(coords).long()
    return x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def mask_coords(mask):
    """Active sites of a mask, sorted by linear index: (n, 4) int32."""
    return torch.nonzero(mask[:, 0] > 0).to(torch.int32).numpy()


def dense_conv(x, mask, weight, bias, geom, subm):
    """One spconv convolution on (x, mask); weight (Cout, kD, kH, kW, Cin).  Returns (y, mask_out), y zero at inactive sites."""
    k, s, p = geom
    w = weight.to(x.dtype).permute(0, 4, 1, 2, 3).contiguous()
    b = None if bias is None else bias.to(x.dtype)
    if subm:
        return F.conv3d(x, w, b, padding=tuple(kk // 2 for kk in k)) * mask, mask
    mo = (F.max_pool3d(mask, k, s, p) > 0).to(x.dtype)
    return F.conv3d(x, w, b, stride=s, padding=p) * mo, mo


def dense_bn(y, mask, bn, eps):
    """Eval BatchNorm1d over the feature rows = per channel, at active sites; bn = [gamma, beta, mean, var]."""
    g, b, mean, var = [t.to(y.dtype).view(1, -1, 1, 1, 1) for t in bn]
    return ((y - mean) / torch.sqrt(var + eps) * g + b) * mask


def brute_conv(features, coords, B, grid, weight, bias, geom, subm):
    """Per-site Python loop, float64: (out_coords sorted by linear index, (n_out, Cout) rows).  Checks dense_conv, nothing else."""
    k, s, p = geom
    feats = features.double().numpy()
    w = weight.double().numpy()
    coords = np.asarray(coords)
    row = {tuple(c): i for i, c in enumerate(coords.tolist())}
    if subm:
        s, p = (1, 1, 1), tuple(kk // 2 for kk in k)
        outs = np.array(sorted(row), np.int32).reshape(-1, 4)
    else:
        outs = out_coords_ref(coords, B, grid, geom)
    in_grid = grid
    res = np.zeros((len(outs), w.shape[0]))
    for o, (b, oz, oy, ox) in enumerate(outs.tolist()):
        for tz, ty, tx in itertools.product(range(k[0]), range(k[1]), range(k[2])):
            z, y, x = oz * s[0] - p[0] + tz, oy * s[1] - p[1] + ty, ox * s[2] - p[2] + tx
            if not (0 <= z < in_grid[0] and 0 <= y < in_grid[1] and 0 <= x < in_grid[2]):
                continue
            j = row.get((b, z, y, x))
            if j is not None:
                res[o] += w[:, tz, ty, tx, :] @ feats[j]
        if bias is not None:
            res[o] += bias.double().numpy()
    return outs, torch.from_numpy(res)


# ---- the whole backbone -------------------------------------------------------------------------------------------
def _bn_tensors(bn):
    return [bn.weight.detach(), bn.bias.detach(), bn.running_mean.detach(), bn.running_var.detach()]


def _block(x, mask, blk):
    h, _ = dense_conv(x, mask, blk.conv1.weight.detach(), blk.conv1.bias.detach(), SUBM, True)
    h = torch.relu(dense_bn(h, mask, _bn_tensors(blk.bn1), blk.bn1.eps))
    o, _ = dense_conv(h, mask, blk.conv2.weight.detach(), blk.conv2.bias.detach(), SUBM, True)
    return torch.relu(dense_bn(o, mask, _bn_tensors(blk.bn2), blk.bn2.eps) + x) * mask


def reference_forward(module, features, coords, B, input_shape, dtype):
    """SpMiddleResNetFHD.forward restated densely on the CPU in `dtype` from the module's own tensors.  Returns
    (ret (B, C * D, H, W), {name: (dense (B, C, D, H, W), mask)} for conv1 .. conv4 and 'ret')."""
    grid = tuple(int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0]))
    x, mask = to_dense(torch.as_tensor(features).to(dtype), coords, B, grid)
    levels = {}
    with torch.no_grad():
        c0, n0 = module.conv_input[0], module.conv_input[1]
        x, _ = dense_conv(x, mask, c0.weight.detach(), None, SUBM, True)
        x = torch.relu(dense_bn(x, mask, _bn_tensors(n0), n0.eps))
        for blk in module.conv1:
            x = _block(x, mask, blk)
        levels["conv1"] = (x, mask)
        for name in ("conv2", "conv3", "conv4", "extra_conv"):
            seq = getattr(module, name)
            conv, bn = seq[0], seq[1]
            x, mask = dense_conv(x, mask, conv.weight.detach(), None, (conv.kernel_size, conv.stride, conv.padding), False)
            x = torch.relu(dense_bn(x, mask, _bn_tensors(bn), bn.eps))
            for blk in list(seq)[3:]:
                x = _block(x, mask, blk)
            levels["ret" if name == "extra_conv" else name] = (x, mask)
    Bn, C, D, H, W = x.shape
    return x.reshape(Bn, C * D, H, W), levels


def randomize(module, gen, gain=1.0):
    """Seeded, non-trivial tensors for every layer: weights ~ N(0, gain / fan_in), small biases, BatchNorm statistics around the
    identity.  The backbone's default init is not the reference's (no RNG parity is claimed), so tests bring their own."""
    from shasta_amd.backbone import _SparseConv
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, _SparseConv):
                fan = m.in_channels * int(np.prod(m.kernel_size))
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * float(np.sqrt(gain / fan)))
                if m.bias is not None:
                    m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
            elif isinstance(m, torch.nn.BatchNorm1d):
                n = m.num_features
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=gen))
                m.bias.copy_(0.1 * torch.randn(n, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=gen))
