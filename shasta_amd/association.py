"""`mot_3d.association` call surface (mot_3d/association.py:9-120) with a learned-affinity mode added.

`associate_dets_to_tracks(dets, tracks, mode, asso, dist_threshold, trk_innovation_matrix)` keeps the reference's
argument meaning and return triple `(matches: list of np.ndarray (det_idx, trk_idx), unmatched_dets, unmatched_tracks)`
so SimpleTrack-style bookkeeping (mot_3d/mot.py:149-150,208-209) consumes the result unchanged.  The distance matrix is
`[len(dets), len(tracks)]` (detections are rows: transposed w.r.t. ShaSTA's matched1).

  asso = 'affinity' : dist = 1 - affinity[:n_trk, :n_det].T with `affinity` = matched1 of the Shasta forward for this
                      frame pair (pass it as `affinity=`); this is how the learned matrix plugs into the reference
                      matchers.
  asso = 'euler' / 'm_dis' : L2 / Mahalanobis on the 7-vector [x,y,z,o,l,w,h] with the reference's yaw folding
                      (mot_3d/utils/geometry.py:246-271).
  asso = 'iou' / 'giou' : 1 - rotated 3-D IoU / GIoU for all pairs at once on the GPU (csrc/iou3d.hip, float64).

mode = 'bipartite' solves with scipy on the host by default; with `device=True` the solver is csrc/lsap.hip (scipy's algorithm step for
step, so the same pairs): the IoU / GIoU matrix then goes from its kernel into the solver without leaving the GPU, the other
distances are uploaded once.  `linear_assignment_device` is that solver for any batch of float64 matrices.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment


def _array7(b):
    if hasattr(b, "x"):
        return np.array([b.x, b.y, b.z, b.o, b.l, b.w, b.h], dtype=np.float64)
    return np.asarray(b, dtype=np.float64)[:7]


def compute_m_distance(dets, tracks, trk_innovation_matrix):
    """mot_3d/association.py:87-105 + utils/geometry.py:258-271."""
    D = np.stack([_array7(d) for d in dets]) if len(dets) else np.zeros((0, 7))
    T = np.stack([_array7(t) for t in tracks]) if len(tracks) else np.zeros((0, 7))
    diff = D[:, None, :] - T[None, :, :]
    yaw = diff[..., 3]
    yaw = np.where(yaw > np.pi / 2, yaw - np.pi, yaw)
    yaw = np.where(yaw < -np.pi / 2, yaw + np.pi, yaw)
    diff[..., 3] = yaw
    if trk_innovation_matrix is None:
        return np.sqrt((diff * diff).sum(-1))
    inv = np.stack([np.linalg.inv(m) for m in trk_innovation_matrix])  # (T,7,7)
    return np.sqrt(np.einsum("dti,tij,dtj->dt", diff, inv, diff))


def compute_affinity_distance(dets, tracks, affinity):
    a = np.asarray(affinity, dtype=np.float64)
    return 1.0 - a[:len(tracks), :len(dets)].T


def linear_assignment_device(cost, n=None, m=None):
    """scipy.optimize.linear_sum_assignment on the GPU (csrc/lsap.hip): the same (row_ind, col_ind), index for index.
    cost: one (N, M) matrix or a batch (P, Nmax, Mmax), float64, a CUDA tensor (stays on the device) or a numpy array (one upload);
    n / m: per-problem valid rows / columns of a batch (sequence, array or int32 device tensor; default: the full extent) - cells
    outside n x m are never read.  Returns (row_ind, col_ind) int64 numpy arrays for a single matrix, a list of such pairs for a batch.
    Raises ValueError where scipy does: a NaN or -inf entry, or an infeasible matrix (+inf marks a forbidden pair); more than 1024
    rows or columns per problem raise ShastaHipError.  One launch, one copy back (col_of_row and the status words)."""
    import torch

    from . import hip
    lib = hip.load()
    if not torch.cuda.is_available():
        raise hip.ShastaHipError("linear_assignment_device needs a GPU; there is no CPU fallback")
    if isinstance(cost, torch.Tensor):
        if cost.dtype != torch.float64 or not cost.is_cuda:
            raise ValueError("linear_assignment_device: a float64 CUDA tensor or a numpy array")
        c = cost.contiguous()
        dev = c.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        c = torch.from_numpy(np.ascontiguousarray(cost, dtype=np.float64)).to(dev)
    single = c.dim() == 2
    if single:
        c = c.unsqueeze(0)
    if c.dim() != 3:
        raise ValueError("linear_assignment_device: cost is (N, M) or (P, Nmax, Mmax)")
    P, Nmax, Mmax = c.shape

    def counts(x, full):
        if x is None:
            return torch.full((P,), full, dtype=torch.int32, device=dev)
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        return torch.from_numpy(np.array(np.broadcast_to(np.asarray(x, np.int32).reshape(-1), (P,)))).to(dev)
    nn, mm = counts(n, Nmax), counts(m, Mmax)
    if nn.numel() != P or mm.numel() != P:
        raise ValueError("linear_assignment_device: n / m hold one count per problem")
    if P == 0 or Nmax == 0 or Mmax == 0:
        empty = [(np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in range(P)]
        return empty[0] if single else empty
    out = torch.empty(P * (Nmax + 1), dtype=torch.int32, device=dev)  # col_of_row | status
    with torch.cuda.device(dev):
        hip.check(lib.shasta_lsap_f64(hip.ptr(c), hip.ptr(nn), hip.ptr(mm), P, Nmax, Mmax, hip.ptr(out[:P * Nmax]), hip.ptr(out[P * Nmax:]),
                                      hip.stream_ptr()), "shasta_lsap_f64")
    out_h = out.cpu().numpy()
    col, status = out_h[:P * Nmax].reshape(P, Nmax), out_h[P * Nmax:]
    res = []
    for p in range(P):
        if status[p] == 1:
            raise ValueError("matrix contains invalid numeric entries" + ("" if single else " (problem %d)" % p))
        if status[p] == 2:
            raise ValueError("cost matrix is infeasible" + ("" if single else " (problem %d)" % p))
        rows = np.nonzero(col[p] >= 0)[0]
        res.append((rows.astype(np.int64), col[p][rows].astype(np.int64)))
    return res[0] if single else res


def _iou_distance_device(dets, tracks, asso):
    """The (len(dets), len(tracks)) float64 distance matrix of asso = 'iou' / 'giou' as a device tensor (csrc/iou3d.hip)."""
    import torch

    from . import hip
    lib = hip.load()
    if not torch.cuda.is_available():
        raise hip.ShastaHipError("asso=%r needs a GPU (rotated IoU kernel); there is no CPU fallback" % asso)
    nd, nt = len(dets), len(tracks)
    dev = torch.device("cuda", torch.cuda.current_device())
    D = torch.from_numpy(np.stack([_array7(d) for d in dets])).to(dev)
    T = torch.from_numpy(np.stack([_array7(t) for t in tracks])).to(dev)
    out = torch.empty(nd, nt, dtype=torch.float64, device=dev)
    hip.check(lib.shasta_iou3d_distance_f64(hip.ptr(D), nd, hip.ptr(T), nt, 7, 1 if asso == "giou" else 0, hip.ptr(out),
                                            hip.stream_ptr()), "shasta_iou3d_distance_f64")
    return out


def compute_iou_distance(dets, tracks, asso="iou"):
    """mot_3d/association.py:108-120 for all pairs at once on the GPU (csrc/iou3d.hip, float64): 1 - iou3d / 1 - giou3d.
    There is no CPU path: without a device this raises."""
    from . import hip
    hip.load()
    nd, nt = len(dets), len(tracks)
    if nd == 0 or nt == 0:
        return np.zeros((nd, nt))
    return _iou_distance_device(dets, tracks, asso).cpu().numpy()


def _dist_matrix(dets, tracks, asso, trk_innovation_matrix, affinity):
    if asso == "affinity":
        if affinity is None:
            raise ValueError("asso='affinity' needs the matched1 matrix of this frame pair (affinity=...)")
        return compute_affinity_distance(dets, tracks, affinity)
    if asso == "m_dis":
        return compute_m_distance(dets, tracks, trk_innovation_matrix)
    if asso == "euler":
        return compute_m_distance(dets, tracks, None)
    if asso in ("iou", "giou"):
        return compute_iou_distance(dets, tracks, asso)
    raise ValueError("unknown asso %r" % (asso,))


def bipartite_matcher(dets, tracks, asso, dist_threshold, trk_innovation_matrix, affinity=None, device=False):
    """device=False: scipy on the host.  device=True: the solver of csrc/lsap.hip - same pairs; the 'iou' / 'giou' matrix stays on the
    GPU between its kernel and the solver (the copy that comes back serves the caller's threshold test), other matrices go up once."""
    if device and len(dets) and len(tracks):
        if asso in ("iou", "giou"):
            on_dev = _iou_distance_device(dets, tracks, asso)
            r, c = linear_assignment_device(on_dev)
            dist = on_dev.cpu().numpy()
        else:
            dist = _dist_matrix(dets, tracks, asso, trk_innovation_matrix, affinity)
            r, c = linear_assignment_device(dist)
        return np.stack([r, c], axis=1), dist
    dist = _dist_matrix(dets, tracks, asso, trk_innovation_matrix, affinity)
    r, c = linear_sum_assignment(dist)
    return np.stack([r, c], axis=1), dist


def greedy_matcher(dets, tracks, asso, dist_threshold, trk_innovation_matrix, affinity=None):
    """Global argsort of the flattened matrix, first come first served (mot_3d/association.py:52-84)."""
    dist = _dist_matrix(dets, tracks, asso, trk_innovation_matrix, affinity)
    nd, nt = dist.shape
    det_of_trk, trk_of_det, matched = [-1] * nt, [-1] * nd, []
    for idx in np.argsort(dist.reshape(-1)):
        d, t = int(idx // nt), int(idx % nt)
        if det_of_trk[t] == -1 and trk_of_det[d] == -1:
            det_of_trk[t], trk_of_det[d] = d, t
            matched.append([d, t])
    matched = np.asarray(matched) if matched else np.empty((0, 2))
    return matched, dist


def associate_dets_to_tracks(dets, tracks, mode, asso, dist_threshold=0.9, trk_innovation_matrix=None, affinity=None, device=False):
    """device=True (mode='bipartite' only): the assignment is solved on the GPU, see bipartite_matcher."""
    if mode == "bipartite":
        matched, dist = bipartite_matcher(dets, tracks, asso, dist_threshold, trk_innovation_matrix, affinity, device=device)
    elif mode == "greedy":
        matched, dist = greedy_matcher(dets, tracks, asso, dist_threshold, trk_innovation_matrix, affinity)
    else:
        raise ValueError("unknown mode %r" % (mode,))
    unmatched_dets = [d for d in range(len(dets)) if d not in matched[:, 0]]
    unmatched_tracks = [t for t in range(len(tracks)) if t not in matched[:, 1]]
    matches = []
    for m in matched:
        if dist[int(m[0]), int(m[1])] > dist_threshold:
            unmatched_dets.append(m[0])
            unmatched_tracks.append(m[1])
        else:
            matches.append(m.reshape(2))
    return matches, np.array(unmatched_dets), np.array(unmatched_tracks)
