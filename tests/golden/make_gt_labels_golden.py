"""Generates tests/golden/gt_labels_golden.json.gz: what the REFERENCE's label construction produces for the seeded synthetic scenes
of tests/gt_label_scenes.py - `associate` of preprocessing/gt_association/associate.py, loaded by file location, and the frame body of
preprocessing/make_gt_shasta.py `main` (from `frame_dets = ...` through the `if prev_sample_token == ''` block).  That body is inline
code of a loop that needs the nuScenes devkit around it, so it is run IN PLACE: the statements are located in the parsed source with
`ast`, compiled from the reference file itself and executed per frame with synthetic lists; no reference text is copied.  The fixture
holds inputs (numbers and strings) and, as indices, each frame's tp_ind_pairs / fn_inds and each emitted frame's one-hot column per
previous detection and newborn flags - no dense matrices.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gt_labels_golden.py
"""
import ast
import gzip
import importlib.util
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
from tests.gt_label_scenes import DET_NAMES, GT_NAMES, golden_scenes  # noqa: E402

SRC = os.path.join(ref_import.REF_ROOT, "preprocessing", "make_gt_shasta.py")
THRESHOLD = 2.0


def reference_associate():
    ref_import._install_stubs()
    if ref_import.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REF_ROOT)
    spec = importlib.util.spec_from_file_location("_ref_gt_associate", os.path.join(ref_import.REF_ROOT, "preprocessing", "gt_association", "associate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_frame_code():
    tree = ast.parse(open(SRC).read(), SRC)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    loop = next(n for n in ast.walk(main) if isinstance(n, ast.While))

    def assigns(stmt, name):
        return isinstance(stmt, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in stmt.targets)
    first = next(i for i, s in enumerate(loop.body) if assigns(s, "frame_dets"))
    last = next(i for i, s in enumerate(loop.body) if isinstance(s, ast.If) and any(isinstance(n, ast.Name) and n.id == "prev_sample_token"
                                                                                   for n in ast.walk(s.test)))
    return compile(ast.Module(body=loop.body[first:last + 1], type_ignores=[]), SRC, "exec")


def main():
    A = reference_associate()
    from mot_3d.data_protos import BBox
    code = reference_frame_code()

    def boxes(xy, score=None):
        out = []
        for i, p in enumerate(xy):
            b = BBox(x=float(p[0]), y=float(p[1]), z=0.0, h=1.5, w=2.0, l=4.0, o=0.0)
            if score is not None:
                b.s = float(score[i])
            out.append(b)
        return out

    count = dict(match=0, dead=0, fn=0, newborn=0, at_threshold=0, tied_minimum=0, tied_match=0)
    scenes_out = {}
    for name, frames in golden_scenes().items():
        dets = [boxes(f["det_xy"], f["det_score"]) for f in frames]
        inst_types = [f["det_types"] for f in frames]
        gt_bboxes = [boxes(f["gt_xy"]) for f in frames]
        gt_inst_types = [f["gt_types"] for f in frames]
        gt_ids = [f["gt_ids"] for f in frames]
        frames_out = []
        for t, f in enumerate(frames):
            r = A.associate(gt_bboxes[t], gt_inst_types[t], dets[t], inst_types[t], threshold=THRESHOLD)
            tp_ind_pairs, fn_inds = r[7], r[9]
            o = dict(det_x=f["det_xy"][:, 0].tolist(), det_y=f["det_xy"][:, 1].tolist(), det_score=f["det_score"].tolist(),
                     det_type=[DET_NAMES.index(v) for v in f["det_types"]], gt_x=f["gt_xy"][:, 0].tolist(), gt_y=f["gt_xy"][:, 1].tolist(),
                     gt_type=[GT_NAMES.index(v) for v in f["gt_types"]], gt_id=f["gt_ids"], emit=int(f["emit"]), has_prev=int(f["has_prev"]),
                     tp_ind_pairs=[[int(k), int(g)] for k, g in tp_ind_pairs.items()], fn_inds=[int(g) for g in fn_inds])
            if len(dets[t]) and len(gt_bboxes[t]):  # what the fixture exercises, from the reference's own distance matrix
                D = A.l2(gt_bboxes[t], dets[t])
                count["at_threshold"] += int((D == THRESHOLD).sum())
                free = np.ones(len(gt_bboxes[t]), dtype=bool)
                # every visited detection (descending score, larger index first): the minimum over the boxes it could still take
                for k in sorted(range(len(dets[t])), key=lambda i: (dets[t][i].s, i), reverse=True):
                    ok = free & np.array([inst_types[t][k] in g for g in gt_inst_types[t]])
                    if ok.any() and (D[ok, k] == D[ok, k].min()).sum() > 1:
                        count["tied_minimum"] += 1
                        count["tied_match"] += int(D[ok, k].min() < THRESHOLD)  # ... and the tie rule decides the pair
                    if k in tp_ind_pairs:
                        free[tp_ind_pairs[k]] = False
            if f["emit"]:
                env = dict(dets=dets, inst_types=inst_types, gt_bboxes=gt_bboxes, gt_inst_types=gt_inst_types, gt_ids=gt_ids, frame_index=t,
                           frame_data={"prev": "x" if f["has_prev"] else ""}, thres=THRESHOLD, associate=A.associate, np=np)
                exec(code, env)
                assert env["tp_ind_pairs"] == tp_ind_pairs and env["fn_inds"] == fn_inds
                matched, newborn = env["matched"], env["newborn"]
                o["newborn"] = [int(v) for v in newborn]
                assert np.array_equal(newborn, np.array(o["newborn"], dtype=np.float64)) and newborn.shape == (len(dets[t]),)
                count["newborn"] += int(newborn.sum())
                if matched is None:
                    o["col_of_prev"] = None
                else:
                    K = len(dets[t])
                    assert matched.shape == (len(dets[t - 1]), K + 2) and ((matched == 0) | (matched == 1)).all() and (matched.sum(axis=1) == 1).all()
                    col = matched.argmax(axis=1) if matched.size else np.zeros(0, dtype=int)
                    o["col_of_prev"] = [int(c) for c in col]
                    count["match"] += int((col < K).sum())
                    count["dead"] += int((col == K).sum())
                    count["fn"] += int((col == K + 1).sum())
            frames_out.append(o)
        scenes_out[name] = frames_out
    print(count)
    assert min(count["match"], count["dead"], count["fn"], count["newborn"]) >= 50, count
    assert count["at_threshold"] >= 1 and count["tied_minimum"] >= 1 and count["tied_match"] >= 1, count
    out = dict(threshold=THRESHOLD, det_names=DET_NAMES, gt_names=GT_NAMES, scenes=scenes_out)
    path = os.path.join(HERE, "gt_labels_golden.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
