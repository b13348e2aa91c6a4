"""Time the CenterPoint head at the shipped shape - B = 1, a 512 x 180 x 180 neck map, the six nuScenes tasks - on the hand-written kernels
(CenterHead.forward: csrc/neck.hip layers + csrc/head.hip) and, with the same weights in the same process, through the module's own nn
layers (CenterHead.forward_layers: MIOpen); then `predict` (decode, sort, batched NMS) on the kernel path's maps.  One HIP event pair per
run after a warm-up, the median of --runs runs (at least 20).  Writes profiles/head_timing.txt and prints it.

    python tools/time_head.py [--runs 20] [--warmup 5] [--hw 180] [--out profiles/head_timing.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
import shasta_amd  # noqa: E402
from shasta_amd import hip  # noqa: E402

TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["truck", "construction_vehicle"]),
         dict(num_class=2, class_names=["bus", "trailer"]), dict(num_class=1, class_names=["barrier"]),
         dict(num_class=2, class_names=["motorcycle", "bicycle"]), dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]
TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500,
                nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2),
                score_threshold=0.1, pc_range=[-54, -54], out_size_factor=8, voxel_size=[0.075, 0.075])


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hw", type=int, default=180)
    ap.add_argument("--out", default=os.path.join("profiles", "head_timing.txt"))
    a = ap.parse_args()
    a.runs = max(a.runs, 20)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    head = shasta_amd.build_head(dict(type="CenterHead", in_channels=[512], tasks=TASKS)).eval().to(dev)
    H = W = a.hw
    x = torch.relu(torch.randn(1, 512, H, W, device=dev))
    prop = torch.cuda.get_device_properties(0)
    box = "%s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, torch.__version__,
                                                 torch.version.hip)
    lines = ["CenterHead at B = 1, 512 x %d x %d, six nuScenes tasks; %s; median (min .. max) of %d runs after %d warm-up runs, one HIP event pair"
             " per run" % (H, W, box, a.runs, a.warmup)]
    npix = H * W
    useful = 2 * 9 * npix * (512 * 64 + sum(64 * 384 + 64 * (10 + t["num_class"]) for t in TASKS))
    executed_final = 2 * 9 * npix * 64 * 16 * 6 * len(TASKS)
    lines.append("useful FLOP %.2f G (shared_conv %.2f, first convs %.2f, final convs %.3f); the final convs execute %.2f GFLOP on 16-row MFMAs"
                 % (useful / 1e9, 2 * 9 * npix * 512 * 64 / 1e9, 2 * 9 * npix * 64 * 384 * len(TASKS) / 1e9,
                    2 * 9 * npix * 64 * sum(10 + t["num_class"] for t in TASKS) / 1e9, executed_final / 1e9))
    with torch.no_grad():
        out = head(x)
        assert head._packed is not None, "the kernel path was not taken"
        t_k = median_ms(lambda: head(x), a.runs, a.warmup)
        t_nn = median_ms(lambda: head.forward_layers(x), a.runs, a.warmup)
        lines.append("forward, kernels (neck.hip layers + head.hip)   %8.3f ms (%.3f .. %.3f)  %.1f TFLOP/s useful" % (t_k + (useful / t_k[0] / 1e9,)))
        lines.append("forward, forward_layers (torch nn: MIOpen)      %8.3f ms (%.3f .. %.3f)  %.1f TFLOP/s useful" % (t_nn + (useful / t_nn[0] / 1e9,)))
        # the three kinds of launches on their own
        lib, st = hip.load(), hip.stream_ptr()
        shared, tasks = head._packed
        s_map, t_map = head._bufs
        first, final, widths, names, chans = tasks[1]
        raw = torch.empty(1, sum(chans), H, W, device=dev)
        t = median_ms(lambda: hip.check(lib.shasta_neck_layer_f32(hip.ptr(x), 1, 512, H, W, hip.ptr(shared), shared.numel(), 0, 64, hip.ptr(s_map), 64, 0,
                                                                  st), "layer"), a.runs, a.warmup)
        lines.append("  shared_conv 512 -> 64 (one launch)            %8.3f ms (%.3f .. %.3f)" % t)
        t = median_ms(lambda: hip.check(lib.shasta_neck_layer_f32(hip.ptr(s_map), 1, 64, H, W, hip.ptr(first), first.numel(), 0, 384, hip.ptr(t_map), 384,
                                                                  0, st), "layer"), a.runs, a.warmup)
        lines.append("  first convs of a task 64 -> 384 (one launch)  %8.3f ms (%.3f .. %.3f)" % t)
        t = median_ms(lambda: hip.check(lib.shasta_head_final_f32(hip.ptr(t_map), 1, 6, widths, H, W, hip.ptr(final), final.numel() * 4, hip.ptr(raw), st),
                                        "final"), a.runs, a.warmup)
        lines.append("  final convs of a task 6 x 64 -> 12 (one launch)%7.3f ms (%.3f .. %.3f)" % t)
        # predict: random weights give arbitrary maps (every task fills its nms_post_max_size)
        dets = head.predict({}, out, TEST_CFG)
        t = median_ms(lambda: head.predict({}, out, TEST_CFG), a.runs, a.warmup)
        lines.append("predict (decode, sort, batched NMS, one host copy) %6.3f ms (%.3f .. %.3f); %d detections"
                     % (t + (int(dets[0]["scores"].shape[0]),)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
