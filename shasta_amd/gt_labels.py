"""Ground-truth affinity labels from detections and ground-truth boxes: the label files `frames.FramePairs.load` reads
(`<labels_path>/<token>.npz`: matched (N_prev, K+2), newborn (K,)), restated from preprocessing/make_gt_shasta.py:81-157 and
preprocessing/gt_association/associate.py:6-80,107-113 (`distance_type="l2"`).

Per frame (`associate`): detections are visited in descending score order, of equal scores the larger index first; each takes the
nearest ground-truth box that is not yet taken and whose type string contains the detection's type (Python's `in`), the lowest index
among equal distances, and only if the distance is below the threshold (strict).  dist = sqrt(dx*dx + dy*dy) in float64 with every
operation rounded (np.linalg.norm over two elements); squared distances would not do, two sums can share a square root.

Per frame pair (`scene_labels`): a row of `matched` is one-hot - the current detection whose ground-truth id the previous detection
held, K = dead track, K+1 = false negative (the id is in the current frame, no detection took it); newborn = a matched detection whose
id no previous matched detection held.  A frame that is not emitted still serves as the previous frame of the next one.

`device=True` runs csrc/gt_labels.hip: every frame of every scene of the call in one `shasta_gt_labels_f64` (one wavefront per
frame), one copy back of three int32 arrays, and the one-hot columns are expanded to the dense float64 matrices on the host.
`device=False` is the same rule in numpy.  Both give the reference's matrices entry for entry (tests/test_gt_labels.py).

A frame is a dict: det_xy (K, 2), det_score (K,), det_types (K values), gt_xy (G, 2), gt_types (G values), gt_ids (G values),
optional emit (default True) and has_prev (default: not the first frame of its scene); `frame()` builds one from box lists.
"""
import os

import numpy as np

MAX_DET, MAX_GT = 1024, 512  # csrc/gt_labels.hip GT_CAP_DET / GT_CAP_GT


def _xy_score(boxes, need_score):
    """Boxes with .x .y .s, or rows [x, y, ..., score]."""
    xy, score = np.zeros((len(boxes), 2)), np.zeros(len(boxes))
    for i, b in enumerate(boxes):
        if hasattr(b, "x"):
            xy[i] = (b.x, b.y)
            if need_score:
                score[i] = b.s
        else:
            xy[i] = (b[0], b[1])
            if need_score:
                score[i] = b[-1]
    return xy, score


def frame(dets, det_types, gt_boxes, gt_types, gt_ids, emit=True, has_prev=None):
    """A frame for `scene_labels` from the lists make_gt_shasta.py holds per frame (detections with a score, ground-truth boxes)."""
    det_xy, det_score = _xy_score(dets, True)
    gt_xy, _ = _xy_score(gt_boxes, False)
    f = dict(det_xy=det_xy, det_score=det_score, det_types=list(det_types), gt_xy=gt_xy, gt_types=list(gt_types), gt_ids=list(gt_ids),
             emit=emit)
    if has_prev is not None:
        f["has_prev"] = has_prev
    return f


def _visit_order(score):
    """sorted((v, i))[::-1]: descending score, of equal scores the larger index first."""
    return [i for (v, i) in sorted((v, i) for (i, v) in enumerate(score))][::-1]


def _compat(det_types, gt_types):
    """Python's `pred_type in gt_type`, evaluated once per pair of distinct values: (det type index (K,), gt type index (G,),
    table (distinct det types, distinct gt types) bool)."""
    dvals, gvals = {}, {}
    dt = np.array([dvals.setdefault(t, len(dvals)) for t in det_types], dtype=np.int64).reshape(-1)
    gt = np.array([gvals.setdefault(t, len(gvals)) for t in gt_types], dtype=np.int64).reshape(-1)
    table = np.zeros((len(dvals), len(gvals)), dtype=bool)
    for d, i in dvals.items():
        for g, j in gvals.items():
            table[i, j] = d in g
    return dt, gt, table


def _associate_host(det_xy, det_score, det_tid, gt_xy, gt_tid, table, threshold):
    """gt_of_det (K,) int: the ground-truth box of every detection or -1, and the visiting order."""
    K, G = len(det_xy), len(gt_xy)
    gt_of_det = np.full(K, -1, dtype=np.int64)
    if K == 0 or G == 0:
        return gt_of_det, []
    order = _visit_order([float(s) for s in det_score])
    free = np.ones(G, dtype=bool)
    for k in order:
        cand = np.nonzero(free & table[det_tid[k]][gt_tid])[0]
        if len(cand) == 0:
            continue
        ex, ey = gt_xy[cand, 0] - det_xy[k, 0], gt_xy[cand, 1] - det_xy[k, 1]
        d = np.sqrt(ex * ex + ey * ey)
        j = int(np.argmin(d))  # the first of equal minima: the lowest index
        if d[j] < threshold:
            free[cand[j]] = False
            gt_of_det[k] = cand[j]
    return gt_of_det, order


def associate(gt_boxes, gt_types, pred_boxes, pred_types, threshold, distance_type="l2"):
    """preprocessing/gt_association/associate.py:6-80 - the same arguments and the same 10-tuple (tp, tp_matches, fp, fn, tp_types,
    fp_types, fn_types, tp_ind_pairs {detection index: ground-truth index}, fp_inds, fn_inds), lists in visiting order."""
    if distance_type != "l2":
        raise NotImplementedError("distance_type=%r: only 'l2' is implemented - the reference's '3D-IOU' branch calls box3d_overlap and "
                                  "torch, which its module never imports, so there is no behaviour to reproduce" % (distance_type,))
    if len(gt_boxes) == 0 or len(pred_boxes) == 0:
        return [], [], pred_boxes, gt_boxes, [], pred_types, gt_types, {}, list(range(len(pred_boxes))), list(range(len(gt_boxes)))
    det_xy, det_score = _xy_score(pred_boxes, True)
    gt_xy, _ = _xy_score(gt_boxes, False)
    _check_finite(det_xy, det_score, gt_xy)
    dt, gt, table = _compat(pred_types, gt_types)
    gt_of_det, order = _associate_host(det_xy, det_score, dt, gt_xy, gt, table, threshold)
    tp, tp_matches, fp, tp_types, fp_types, tp_ind_pairs, fp_inds = [], [], [], [], [], {}, []
    for k in order:
        g = int(gt_of_det[k])
        if g >= 0:
            tp.append(pred_boxes[k])
            tp_matches.append(gt_boxes[g])
            tp_types.append(pred_types[k])
            tp_ind_pairs[k] = g
        else:
            fp.append(pred_boxes[k])
            fp_types.append(pred_types[k])
            fp_inds.append(k)
    taken = set(tp_ind_pairs.values())
    fn_inds = [g for g in range(len(gt_boxes)) if g not in taken]
    return (tp, tp_matches, fp, [gt_boxes[g] for g in fn_inds], tp_types, fp_types, [gt_types[g] for g in fn_inds], tp_ind_pairs, fp_inds,
            fn_inds)


def _check_finite(det_xy, det_score, gt_xy):
    if not (np.isfinite(det_xy).all() and np.isfinite(det_score).all() and np.isfinite(gt_xy).all()):
        raise ValueError("gt_labels: a score or coordinate is not finite (the reference's order and minimum are undefined for NaN)")


def _prepare(scenes):
    """Validates and flattens the frames of all scenes.  Returns a dict of flat arrays (frame f = rows det_off[f]:det_off[f+1] /
    gt_off[f]:gt_off[f+1]) with type values numbered over the whole call and ids numbered per scene by first occurrence."""
    det_xy, det_score, det_types, gt_xy, gt_types, gt_id = [], [], [], [], [], []
    det_off, gt_off, has_prev, emit, scene_of = [0], [0], [], [], []
    for s, frames in enumerate(scenes):
        ids = {}
        for t, fr in enumerate(frames):
            dxy = np.asarray(fr["det_xy"], dtype=np.float64).reshape(-1, 2)
            sc = np.asarray(fr["det_score"], dtype=np.float64).reshape(-1)
            gxy = np.asarray(fr["gt_xy"], dtype=np.float64).reshape(-1, 2)
            if not (len(sc) == len(dxy) == len(fr["det_types"]) and len(gxy) == len(fr["gt_types"]) == len(fr["gt_ids"])):
                raise ValueError("gt_labels: scene %d frame %d: lengths of boxes, scores, types and ids differ" % (s, t))
            _check_finite(dxy, sc, gxy)
            if len(set(fr["gt_ids"])) != len(fr["gt_ids"]):
                raise ValueError("gt_labels: scene %d frame %d: a ground-truth id occurs twice in one frame - the reference then links "
                                 "whichever box comes first in its lists, its labels depend on list order" % (s, t))
            hp = bool(fr.get("has_prev", t > 0))
            if hp and t == 0:
                raise ValueError("gt_labels: scene %d: the first frame of a scene has no previous frame" % s)
            det_xy.append(dxy)
            det_score.append(sc)
            gt_xy.append(gxy)
            det_types.extend(fr["det_types"])
            gt_types.extend(fr["gt_types"])
            gt_id.extend(ids.setdefault(i, len(ids)) for i in fr["gt_ids"])
            det_off.append(det_off[-1] + len(dxy))
            gt_off.append(gt_off[-1] + len(gxy))
            has_prev.append(hp)
            emit.append(bool(fr.get("emit", True)))
            scene_of.append(s)
    det_tid, gt_tid, table = _compat(det_types, gt_types)
    cat = lambda parts, w: np.concatenate(parts).reshape((-1,) + w) if parts else np.zeros((0,) + w)  # noqa: E731
    return dict(det_xy=cat(det_xy, (2,)), det_score=cat(det_score, ()), det_tid=det_tid, gt_xy=cat(gt_xy, (2,)), gt_tid=gt_tid,
                gt_id=np.array(gt_id, dtype=np.int64).reshape(-1), table=table, det_off=np.array(det_off), gt_off=np.array(gt_off),
                has_prev=np.array(has_prev, dtype=bool), emit=np.array(emit, dtype=bool), scene_of=scene_of)


def _labels_host(p, threshold):
    """gt_of_det, col_of_prev, newborn as the kernels write them (flat over the detections of the call)."""
    D, F = len(p["det_score"]), len(p["emit"])
    gt_of_det, col_of_prev, newborn = np.full(D, -1, dtype=np.int64), np.full(D, -1, dtype=np.int64), np.zeros(D, dtype=np.int64)
    for f in range(F):
        d, g = slice(p["det_off"][f], p["det_off"][f + 1]), slice(p["gt_off"][f], p["gt_off"][f + 1])
        gt_of_det[d], _ = _associate_host(p["det_xy"][d], p["det_score"][d], p["det_tid"][d], p["gt_xy"][g], p["gt_tid"][g], p["table"], threshold)
    for f in range(F):
        if not p["emit"][f]:
            continue
        d0, d1, g0 = p["det_off"][f], p["det_off"][f + 1], p["gt_off"][f]
        K = d1 - d0
        cur = gt_of_det[d0:d1]
        det_of_id = {int(p["gt_id"][g0 + g]): k for k, g in enumerate(cur) if g >= 0}  # ids of the matched current detections
        if not p["has_prev"][f]:
            newborn[d0:d1] = cur >= 0
            continue
        p0, pg0 = p["det_off"][f - 1], p["gt_off"][f - 1]
        prev = gt_of_det[p0:d0]
        prev_ids = {int(p["gt_id"][pg0 + g]) for g in prev if g >= 0}
        cur_ids = {int(i) for i in p["gt_id"][g0:p["gt_off"][f + 1]]}
        for i, k in det_of_id.items():
            newborn[d0 + k] = i not in prev_ids
        for n, g in enumerate(prev):
            i = int(p["gt_id"][pg0 + g]) if g >= 0 else None
            if i is None or i not in cur_ids:
                col_of_prev[p0 + n] = K  # dead: a false positive, or its object has left the ground truth
            else:
                col_of_prev[p0 + n] = det_of_id.get(i, K + 1)  # the id is here: its detection, or a false negative
    return gt_of_det, col_of_prev, newborn


def _labels_device(p, threshold):
    import torch

    from . import hip
    lib = hip.load()
    if not torch.cuda.is_available():
        raise hip.ShastaHipError("gt_labels with device=True needs a GPU; there is no CPU fallback (device=False is the host restatement)")
    D, G, F, T = len(p["det_score"]), len(p["gt_id"]), len(p["emit"]), p["table"].shape[0]
    if p["table"].shape[1] > 64:
        raise ValueError("gt_labels: more than 64 distinct ground-truth type values in one call (the type test is a 64-bit mask)")
    max_det, max_gt = int(np.diff(p["det_off"]).max(initial=0)), int(np.diff(p["gt_off"]).max(initial=0))
    masks = (p["table"].astype(np.uint64) << np.arange(p["table"].shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    # two uploads: the float64 side (the masks travel as their bit patterns, which keeps them 8-byte aligned) and the int32 side
    f64 = np.concatenate([p["det_xy"].reshape(-1), p["det_score"], p["gt_xy"].reshape(-1), masks.view(np.float64)])
    i32 = np.concatenate([p["det_tid"], p["det_off"], p["gt_tid"], p["gt_id"], p["gt_off"], p["has_prev"], p["emit"]]).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    f64_d, i32_d = torch.from_numpy(f64).to(dev), torch.from_numpy(i32).to(dev)
    out = torch.empty(3 * D, dtype=torch.int32, device=dev)  # gt_of_det | col_of_prev | newborn

    def part(buf, sizes):
        ptrs, at = [], 0
        for n in sizes:
            ptrs.append(hip.ptr(buf[at:at + n]) if n else None)
            at += n
        return ptrs
    det_xy, det_score, gt_xy, mask = part(f64_d, [2 * D, D, 2 * G, T])
    det_tid, det_off, gt_tid, gt_id, gt_off, has_prev, emit = part(i32_d, [D, F + 1, G, G, F + 1, F, F])
    gt_of_det, col_of_prev, newborn = part(out, [D, D, D])
    with torch.cuda.device(dev):
        hip.check(lib.shasta_gt_labels_f64(det_xy, det_score, det_tid, det_off, gt_xy, gt_tid, gt_id, gt_off, mask, T, has_prev, emit, F, D, G,
                                           max_det, max_gt, float(threshold), gt_of_det, col_of_prev, newborn, hip.stream_ptr()),
                  "shasta_gt_labels_f64")
    out_h = out.cpu().numpy().astype(np.int64)
    return out_h[:D], out_h[D:2 * D], out_h[2 * D:]


def _expand(p, col_of_prev, newborn):
    """Per scene, per emitted frame: (matched (N, K+2) float64 or None, newborn (K,) float64) as make_gt_shasta.py:157 saves them."""
    res = [[] for _ in range(max(p["scene_of"], default=-1) + 1)]
    for f, s in enumerate(p["scene_of"]):
        if not p["emit"][f]:
            continue
        d0, d1 = p["det_off"][f], p["det_off"][f + 1]
        matched = None
        if p["has_prev"][f]:
            p0 = p["det_off"][f - 1]
            matched = np.zeros((d0 - p0, d1 - d0 + 2))
            matched[np.arange(d0 - p0), col_of_prev[p0:d0]] = 1.0
        res[s].append((matched, newborn[d0:d1].astype(np.float64)))
    return res


def split_labels(scenes, threshold=2.0, device=True):
    """Labels of many scenes (each a list of frames in order) - on the device in one launch.  Returns, per scene, the list of
    (matched, newborn) of its emitted frames; see `scene_labels`."""
    scenes = [list(frames) for frames in scenes]
    p = _prepare(scenes)
    if threshold != threshold:
        raise ValueError("gt_labels: the threshold is NaN")
    _, col_of_prev, newborn = (_labels_device if device else _labels_host)(p, threshold)
    res = _expand(p, col_of_prev, newborn)
    return res + [[] for _ in range(len(scenes) - len(res))]


def scene_labels(frames, threshold=2.0, device=True):
    """The label matrices of one scene: per emitted frame (matched (N_prev, K+2) float64 one-hot rows [K current detections | dead |
    false negative], or None for a frame without a previous one; newborn (K,) float64), as the reference saves them."""
    return split_labels([frames], threshold, device)[0]


def frame_associations(frames, threshold=2.0, device=True):
    """Per frame of a scene (emitted or not): (tp_ind_pairs {detection: ground-truth box}, fn_inds) of `associate`."""
    p = _prepare([list(frames)])
    gt_of_det = (_labels_device if device else _labels_host)(p, threshold)[0]
    out = []
    for f in range(len(p["emit"])):
        cur = gt_of_det[p["det_off"][f]:p["det_off"][f + 1]]
        taken = {int(g) for g in cur if g >= 0}
        out.append(({k: int(g) for k, g in enumerate(cur) if g >= 0}, [g for g in range(p["gt_off"][f + 1] - p["gt_off"][f]) if g not in taken]))
    return out


def write_labels(labels_path, tokens, labels):
    """`<labels_path>/<token>.npz` with `matched` and `newborn` (make_gt_shasta.py:157) for the emitted frames of a scene:
    tokens[i] names labels[i].  `frames.FramePairs.load` reads these files."""
    tokens, labels = list(tokens), list(labels)
    if len(tokens) != len(labels):
        raise ValueError("write_labels: %d tokens for %d emitted frames" % (len(tokens), len(labels)))
    os.makedirs(labels_path, exist_ok=True)
    for token, (matched, newborn) in zip(tokens, labels):
        np.savez_compressed(os.path.join(labels_path, token + ".npz"), matched=matched, newborn=newborn)
