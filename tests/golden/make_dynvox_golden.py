"""Fixture generation only (build container): runs the reference's DynamicVoxelEncoder on the CPU and stores inputs and outputs in
tests/golden/dynvox_golden.npz.  Three small batches:
  faces   : points exactly on every lower and upper face of the range, and random points, in two clouds
  crowded : one voxel with 2 500 points (its mean is an in-order float32 sum) among scattered ones
  batch   : three clouds, the middle one empty
Per batch b: b_range (6,), b_voxel (3,), b_offsets (n + 1,), b_points (sum P, ndim), b_voxels, b_coors (int64), b_shape (int32).

    python tests/golden/make_dynvox_golden.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def reference_encoder():
    ref_import.import_shasta()
    return importlib.import_module("det3d.models.readers.dynamic_voxel_encoder").DynamicVoxelEncoder


def faces_batch(rng, rg, ndim):
    lo, hi = np.array(rg[:3], np.float32), np.array(rg[3:], np.float32)
    clouds = []
    for n in (600, 400):
        pts = (rng.rand(n, ndim) * np.concatenate([hi - lo, np.ones(ndim - 3)]) + np.concatenate([lo, np.zeros(ndim - 3)])).astype(np.float32)
        k = 0
        for j in range(3):
            for face in (lo[j], hi[j]):
                pts[k:k + 4, j] = face
                k += 4
        pts[k, :3] = hi  # the far corner: every coordinate equals its extent
        pts[k + 1, :3] = lo
        clouds.append(pts)
    return clouds


def crowded_batch(rng, rg, vs, ndim):
    lo = np.array(rg[:3], np.float32)
    cell = lo + np.array(vs, np.float32) * np.array([17, 9, 3], np.float32)
    crowd = (cell + rng.rand(2500, 3) * np.array(vs) * 0.98 + 0.01 * np.array(vs)).astype(np.float32)
    crowd = np.concatenate([crowd, (rng.rand(2500, ndim - 3) * 200).astype(np.float32)], 1)
    rest = faces_batch(rng, rg, ndim)[0][30:330]
    pts = np.concatenate([crowd, rest])
    return [pts[rng.permutation(len(pts))]]


def main():
    Enc = reference_encoder()
    rng = np.random.RandomState(20260)
    rg, vs = [-4.0, -3.0, -1.0, 4.0, 3.0, 1.0], [0.25, 0.2, 0.4]
    batches = {
        "faces": (rg, vs, faces_batch(rng, rg, 5)),
        "crowded": (rg, vs, crowded_batch(rng, rg, vs, 4)),
        "batch": ([-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], [0.075, 0.075, 0.2],
                  [(rng.randn(700, 5) * [25, 25, 2, 1, 1]).astype(np.float32), np.zeros((0, 5), np.float32),
                   (rng.randn(333, 5) * [40, 40, 3, 1, 1]).astype(np.float32)]),
    }
    out = {}
    torch.set_num_threads(1)
    for name, (r, v, clouds) in batches.items():
        enc = Enc(r, v)
        voxels, coors, shape = enc([torch.from_numpy(c) for c in clouds])
        out[name + "_range"] = np.asarray(r, np.float32)
        out[name + "_voxel"] = np.asarray(v, np.float32)
        out[name + "_offsets"] = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
        out[name + "_points"] = np.concatenate(clouds).astype(np.float32)
        out[name + "_voxels"] = voxels.numpy()
        out[name + "_coors"] = coors.numpy()
        out[name + "_shape"] = np.asarray(shape)
        assert voxels.dtype == torch.float32 and coors.dtype == torch.int64 and np.asarray(shape).dtype == np.int32
        print(name, "points", len(out[name + "_points"]), "voxels", len(voxels), "shape", shape)
    path = os.path.join(HERE, "dynvox_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
