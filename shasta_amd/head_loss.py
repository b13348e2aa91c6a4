"""CenterPoint's head losses - FastFocalLoss on the heatmaps, RegLoss (masked L1) on the box channels - with their gradient
(csrc/center_loss.hip).  The reference ships no source for the head; these are `CenterHead.loss`'s formulas for nuScenes, per task:

    p = clamp(sigmoid(hm_logit), 1e-4, 1 - 1e-4)
    neg = sum_all log(1 - p) p^2 (1 - target)^4          pos = sum_{b,k} mask log(q) (1 - q)^2,  q = p[b, cat[b,k], ind[b,k]]
    num_pos = sum mask (whole batch)                      hm_loss = -(pos + neg) / num_pos, or -neg when num_pos == 0
    pred[b,k,:] = (reg, height, dim, vel, rot)[b, :, ind[b,k]]   (10 channels, the order of anno_box)
    box_loss[c] = sum_{b,k} |pred mask - target mask| / (num_pos + 1e-4)      loc_loss = sum_c box_loss[c] code_weights[c]
    loss = hm_loss + weight loc_loss

  * `CenterLoss` - a torch.autograd.Function for fp32 device tensors: ONE `shasta_center_loss_f32` call serves all tasks, computes the
    losses and, in the same pass over the logits and targets, the gradient of every task's `loss` with respect to the head's raw
    outputs; backward scales the kept gradient tensors by the incoming scalars.  `mask` is a flag (non-zero = 1), as AssignLabel writes it.
    Only `loss` carries a gradient; `hm_loss`, `loc_loss`, `loc_loss_elem` and `num_positive` are returned detached.
  * `composite_loss` - the same formulas as plain torch operations, for everything else: CPU, other dtypes, double backward.
  * `center_loss(preds_dicts, example, weight, code_weights)` picks between them and returns the per-task dicts
    `{loss, hm_loss, loc_loss, loc_loss_elem (10,), num_positive}`, all device tensors."""
import ctypes as C

import torch

from . import hip

BOX_HEADS = ("reg", "height", "dim", "vel", "rot")  # the channel order of anno_box
BOX_WIDTHS = (2, 1, 3, 2, 2)
KEYS = ("hm",) + BOX_HEADS
MAX_BATCH, MAX_TASKS, MAX_TASK_CLASSES, MAX_OBJS, MAX_MAP = 64, 16, 4, 1024, 512  # include/shasta_hip.h SHASTA_CENTER_*


def composite_task_loss(pd, target_hm, anno_box, ind, mask, cat, weight, code_weights):
    """One task as plain torch operations (any device and floating dtype, differentiable to any order)."""
    hm = pd["hm"]
    p = torch.clamp(torch.sigmoid(hm), min=1e-4, max=1 - 1e-4)
    B, Cn, H, W = p.shape
    m = mask.to(p.dtype)
    gt = torch.pow(1 - target_hm.to(p.dtype), 4)
    neg = (torch.log(1 - p) * torch.pow(p, 2) * gt).sum()
    flat = p.reshape(B, Cn, H * W)
    q = flat.gather(2, ind.long()[:, None, :].expand(B, Cn, -1)).gather(1, cat.long()[:, None, :])[:, 0]  # (B, max_objs)
    pos = (torch.log(q) * torch.pow(1 - q, 2) * m).sum()
    num_pos = m.sum()
    hm_loss = torch.where(num_pos == 0, -neg, -(pos + neg) / torch.where(num_pos == 0, torch.ones_like(num_pos), num_pos))
    maps = torch.cat([pd[n] for n in BOX_HEADS], 1).reshape(B, 10, H * W)
    pred = maps.gather(2, ind.long()[:, None, :].expand(B, 10, -1)).transpose(1, 2)  # (B, max_objs, 10)
    elem = torch.abs(pred * m[..., None] - anno_box.to(p.dtype) * m[..., None]).sum((0, 1)) / (num_pos + 1e-4)
    loc = (elem * torch.as_tensor(code_weights, dtype=p.dtype, device=p.device)).sum()
    return dict(loss=hm_loss + weight * loc, hm_loss=hm_loss, loc_loss=loc, loc_loss_elem=elem, num_positive=num_pos)


def composite_loss(preds_dicts, example, weight, code_weights):
    return [composite_task_loss(pd, example["hm"][t], example["anno_box"][t], example["ind"][t], example["mask"][t], example["cat"][t],
                                weight, code_weights) for t, pd in enumerate(preds_dicts)]


def _view_ok(t, width, H, W):
    """(B, width, H, W) fp32 with channels and pixels contiguous: a channel slice of a larger contiguous tensor is."""
    return (t.dtype == torch.float32 and t.is_cuda and t.dim() == 4 and t.shape[1] == width and t.shape[2] == H and t.shape[3] == W
            and t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W and (t.shape[0] == 1 or t.stride(0) >= width * H * W))


class CenterLoss(torch.autograd.Function):
    """forward(weight, code_weights, num_tasks, *tensors): tensors = per task the 6 raw outputs (hm, reg, height, dim, vel, rot), then
    per task the 5 targets (hm, anno_box, ind, mask, cat).  Returns (loss (T,), detail (T, 14)): detail rows are [loss, hm_loss, loc_loss,
    box_loss[0..9], num_pos]; `detail` carries no gradient."""

    @staticmethod
    def forward(ctx, weight, code_weights, T, *tensors):
        raws, tgts = tensors[:6 * T], tensors[6 * T:]
        lib = hip.load()
        B, _, H, W = raws[0].shape
        max_objs = int(tgts[2].shape[1])
        dev = raws[0].device
        wsb = lib.shasta_center_loss_workspace_bytes(T, B)
        if wsb == 0:
            raise hip.ShastaHipError("CenterLoss serves 1..%d tasks and 1..%d samples (got %d, %d)" % (MAX_TASKS, MAX_BATCH, T, B))
        table = (hip.CenterLossTask * T)()
        keep, grads = [], []
        with torch.cuda.device(dev):
            for t in range(T):
                hm, boxes = raws[6 * t], raws[6 * t + 1:6 * t + 6]
                thm, anno, ind, mask, cat = tgts[5 * t:5 * t + 5]
                Cn = int(hm.shape[1])
                hm = hm if _view_ok(hm, Cn, H, W) else hm.contiguous()
                boxes = [b if _view_ok(b, w, H, W) else b.contiguous() for b, w in zip(boxes, BOX_WIDTHS)]
                thm, anno = thm.to(torch.float32).contiguous(), anno.to(torch.float32).contiguous()
                ind, cat, mask = ind.to(torch.int64).contiguous(), cat.to(torch.int64).contiguous(), mask.to(torch.uint8).contiguous()
                if thm.shape != (B, Cn, H, W) or anno.shape != (B, max_objs, 10) or any(v.shape != (B, max_objs) for v in (ind, cat, mask)):
                    raise ValueError("CenterLoss: task %d: targets do not match the outputs' shape" % t)
                g_hm = torch.empty(B, Cn, H, W, dtype=torch.float32, device=dev)
                g_box = torch.empty(B, 10, H, W, dtype=torch.float32, device=dev)
                k = table[t]
                k.hm, k.target_hm, k.anno_box = hm.data_ptr(), thm.data_ptr(), anno.data_ptr()
                k.ind, k.cat, k.mask, k.g_hm, k.g_box = ind.data_ptr(), cat.data_ptr(), mask.data_ptr(), g_hm.data_ptr(), g_box.data_ptr()
                k.hm_stride, k.num_class = (hm.stride(0) if B > 1 else Cn * H * W), Cn
                for i, b in enumerate(boxes):
                    k.box[i] = b.data_ptr()
                    k.box_stride[i] = b.stride(0) if B > 1 else BOX_WIDTHS[i] * H * W
                keep.append((hm, boxes, thm, anno, ind, cat, mask))
                grads += [g_hm, g_box]
            out = torch.empty(T, 14, dtype=torch.float32, device=dev)
            ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
            cw = (C.c_float * 10)(*[float(v) for v in code_weights])
            hip.check(lib.shasta_center_loss_f32(table, T, B, H, W, max_objs, float(weight), cw, hip.ptr(out), hip.ptr(ws), wsb,
                                                 hip.stream_ptr()), "shasta_center_loss_f32")
        del keep  # (the stream orders the kernels before any reuse of these buffers by the caching allocator)
        ctx.T = T
        ctx.save_for_backward(*grads)
        loss = out[:, 0].clone()
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_detail):
        grads = ctx.saved_tensors
        ret = []
        for t in range(ctx.T):
            g_hm, g_box = grads[2 * t], grads[2 * t + 1]
            s = g_loss[t]
            ret.append(g_hm * s)
            gb = g_box * s
            at = 0
            for w in BOX_WIDTHS:
                ret.append(gb[:, at:at + w])
                at += w
        return (None, None, None) + tuple(ret) + (None,) * (5 * ctx.T)


def _kernel_path(preds_dicts, example):
    T = len(preds_dicts)
    if not 1 <= T <= MAX_TASKS:
        return False
    shape = None
    for t, pd in enumerate(preds_dicts):
        hm = pd["hm"]
        if not all(torch.is_tensor(pd[k]) and pd[k].is_cuda and pd[k].dtype == torch.float32 and pd[k].dim() == 4 for k in KEYS):
            return False
        B, Cn, H, W = hm.shape
        if shape is None:
            shape = (B, H, W)
        if (B, H, W) != shape or not (1 <= B <= MAX_BATCH and 1 <= Cn <= MAX_TASK_CLASSES and H <= MAX_MAP and W <= MAX_MAP):
            return False
        if any(pd[n].shape != (B, w, H, W) for n, w in zip(BOX_HEADS, BOX_WIDTHS)):
            return False
        if not all(example[k][t].is_cuda for k in ("hm", "anno_box", "ind", "mask", "cat")):
            return False
        if example["ind"][t].dim() != 2 or not 1 <= example["ind"][t].shape[1] <= MAX_OBJS:
            return False
    return True


def center_loss(preds_dicts, example, weight, code_weights, force_composite=False):
    """preds_dicts: per task {hm, reg, height, dim, vel, rot: (B, channels, H, W)}; example: `hm, anno_box, ind, mask, cat` as lists over
    tasks of batched tensors (what `targets.assign_targets` returns).  -> per task {loss, hm_loss, loc_loss, loc_loss_elem, num_positive}."""
    if len(code_weights) != 10:
        raise ValueError("center_loss: ten code weights, one per anno_box channel (got %d)" % len(code_weights))
    for pd in preds_dicts:
        for k in KEYS:
            if k not in pd:
                raise NotImplementedError("center_loss: the nuScenes heads %s are needed (no %r)" % (KEYS, k))
    if force_composite or not _kernel_path(preds_dicts, example):
        return composite_loss(preds_dicts, example, weight, code_weights)
    T = len(preds_dicts)
    raws = [pd[k] for pd in preds_dicts for k in KEYS]
    tgts = [example[k][t] for t in range(T) for k in ("hm", "anno_box", "ind", "mask", "cat")]
    loss, out = CenterLoss.apply(float(weight), tuple(float(v) for v in code_weights), T, *raws, *tgts)
    return [dict(loss=loss[t], hm_loss=out[t, 1], loc_loss=out[t, 2], loc_loss_elem=out[t, 3:13], num_positive=out[t, 13]) for t in range(T)]
