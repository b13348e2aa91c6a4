"""GPU: the detection head's kernels through the C ABI against torch's CPU float64 (tests/head_helpers.py holds the oracles and bars).

Seams of the kernels: the bias + BatchNorm + ReLU layers are neck layers - a 4 x 32 rectangular tile, or 128 flattened pixels per workgroup
on maps up to 256 columns wide; the final convolutions take 256 flattened pixels per workgroup, 64 per wave, 16 per accumulator; the decode
takes 256 pixels per block, 64 per ballot; the NMS 64 boxes per mask word."""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_helpers as HH

pytestmark = pytest.mark.gpu
E_UNSUPPORTED = -5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _guarded(shape, dev):
    """A NaN-poisoned tensor of `shape` inside a buffer with one guard row (the tensor's last dimension) at either end."""
    n, w = int(np.prod(shape)), int(shape[-1])
    buf = torch.full((n + 2 * w,), float("nan"), device=dev)
    return buf, buf[w:w + n].view(*shape)


def _guards_untouched(buf, shape):
    w = int(shape[-1])
    return bool(torch.isnan(buf[:w]).all()) and bool(torch.isnan(buf[-w:]).all())


def _abi_runners(head, dev, record):
    """check_chain's two callbacks on the C ABI: NaN-poisoned, guarded outputs; every call is made twice and the bits compared."""
    from shasta_amd import hip
    lib = hip.load()

    def twice(call, shape):
        outs = []
        for _ in range(2):
            buf, out = _guarded(shape, dev)
            assert call(out) == 0, lib.shasta_last_error()
            torch.cuda.synchronize()
            assert _guards_untouched(buf, shape), "a write outside the output tensor"
            assert not bool(torch.isnan(out).any()), "an entry of the output was not written"
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "two runs differ"
        record.append(tuple(shape))
        return outs[0].cpu()

    def run_bn_layer(convs, bns, x):
        packed = head._pack_bn_layer(lib, convs, bns, dev)
        xd = x.to(dev).contiguous()
        B, cin, H, W = xd.shape
        cout = sum(c.out_channels for c in convs)
        return twice(lambda out: lib.shasta_neck_layer_f32(hip.ptr(xd), B, cin, H, W, hip.ptr(packed), packed.numel(), 0, cout, hip.ptr(out), cout, 0,
                                                           hip.stream_ptr()), (B, cout, H, W))

    def run_final(convs, x):
        packed = head._pack_final(convs, dev)
        xd = x.to(dev).contiguous()
        B, c, H, W = xd.shape
        widths = (ctypes.c_int * len(convs))(*[cv.out_channels for cv in convs])
        assert lib.shasta_head_final_packed_bytes(len(convs)) == packed.numel() * 4
        return twice(lambda out: lib.shasta_head_final_f32(hip.ptr(xd), B, len(convs), widths, H, W, hip.ptr(packed), packed.numel() * 4, hip.ptr(out),
                                                           hip.stream_ptr()), (B, sum(widths), H, W))

    return run_bn_layer, run_final


def _conv_case(in_channels, tasks, B, H, W, seed):
    dev = _dev()
    head = HH.make_head(in_channels, tasks, seed)
    x = torch.relu(torch.randn(B, in_channels, H, W, generator=torch.Generator().manual_seed(seed + 7)))
    record = []
    raws = HH.check_chain(head, x, *_abi_runners(head, dev, record))
    assert len(raws) == len(tasks) and len(record) == 1 + 2 * len(tasks)
    assert [r.shape[1] for r in raws] == [10 + t["num_class"] for t in tasks]


@pytest.mark.parametrize("in_channels", [8, 24])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (5, 33), (9, 130)])
def test_convolutions_vs_float64(H, W, B, in_channels):
    """shared_conv, the first convolutions of a task as one 384-channel layer, and the final convolutions, each against float64 on its
    own fp32 input, entry by entry, at the bars of head_helpers; outputs NaN-poisoned with guard rows; two runs, the same bits."""
    _conv_case(in_channels, HH.TWO_TASKS, B, H, W, 100 * H + W + B + in_channels)


def test_convolutions_six_nuscenes_tasks():
    _conv_case(24, HH.NUSC_TASKS, 1, 5, 33, 31)


def test_convolutions_512_input_channels():
    _conv_case(512, HH.TWO_TASKS, 1, 9, 130, 32)


def test_refusals_come_before_any_launch():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    w3 = (ctypes.c_int * 2)(2, 3)
    w4 = (ctypes.c_int * 2)(2, 4)
    assert lib.shasta_head_supported(512, 64, 2, w3, 180, 180) == 1
    assert lib.shasta_head_supported(512, 64, 2, w4, 180, 180) == 0      # final width 4
    assert lib.shasta_head_supported(12, 64, 2, w3, 8, 8) == 0            # in_channels % 8
    assert lib.shasta_head_supported(16, 48, 2, w3, 8, 8) == 0            # share_conv_channel % 32
    assert lib.shasta_head_supported(16, 64, 17, (ctypes.c_int * 17)(*[1] * 17), 8, 8) == 0
    assert lib.shasta_head_final_packed_bytes(0) == 0 and lib.shasta_head_final_packed_bytes(17) == 0
    x = torch.zeros(1, 128, 4, 4, device=dev)
    packed = torch.zeros(2 * 2308, device=dev)
    buf, out = _guarded((1, 6, 4, 4), dev)
    st = hip.stream_ptr()
    assert lib.shasta_head_final_f32(hip.ptr(x), 1, 2, w4, 4, 4, hip.ptr(packed), packed.numel() * 4, hip.ptr(out), st) == E_UNSUPPORTED
    assert lib.shasta_head_final_f32(None, 1, 2, w3, 4, 4, hip.ptr(packed), packed.numel() * 4, hip.ptr(out), st) != 0
    assert lib.shasta_head_final_f32(hip.ptr(x), 1, 2, w3, 4, 4, hip.ptr(packed), 2 * 2308 * 4 - 1, hip.ptr(out), st) != 0
    assert lib.shasta_head_final_f32(hip.ptr(x), 65536, 2, w3, 4, 4, hip.ptr(packed), packed.numel() * 4, hip.ptr(out), st) == E_UNSUPPORTED
    cfg = HH.decode_cfg(2, HH.DECODE_CFG)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(64, dtype=torch.int32, device=dev)
    raw = torch.zeros(1, 11, 4, 4, device=dev)  # one channel short of hm's two classes
    assert lib.shasta_head_decode_f32(hip.ptr(raw), 1, 11, 4, 4, ctypes.byref(cfg), 0, None, None, None, None, hip.ptr(cnt), hip.ptr(ws), 256, st) != 0
    assert lib.shasta_head_decode_f32(hip.ptr(raw), 1, 12, 4, 4, ctypes.byref(cfg), 0, None, None, None, None, hip.ptr(cnt), hip.ptr(ws), 0, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and int(cnt) == -7


# ---- decode -----------------------------------------------------------------------------------------------------------

def _decode(raw, num_class, test_cfg, cap=None):
    from shasta_amd import head
    out = head.decode_candidates(raw.to(_dev()).contiguous(), HH.decode_cfg(num_class, test_cfg), cap=cap)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_decoded(got, b, oracle, bars, H, W, test_cfg, what, cap=None):
    n = len(oracle["pixel"])
    assert int(got["count"][b]) == n, (what, int(got["count"][b]), n)
    m = n if cap is None else min(n, cap)
    assert got["pixel"][b, :m].tolist() == oracle["pixel"][:m].tolist(), what + ": kept set or order"
    assert got["label"][b, :m].tolist() == oracle["label"][:m].tolist(), what + ": labels"
    HH.assert_boxes(got["box"][b, :m], got["score"][b, :m], oracle["box"][:m], oracle["score"][:m], bars, W, H, test_cfg, what)
    # nothing past the count (or the capacity)
    assert bool((got["pixel"][b, m:] == -1).all()) and bool(torch.isinf(got["score"][b, m:]).all()) and bool((got["box"][b, m:] == 0).all()), what


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257, 9 * 130])
def test_decode_against_float64(count):
    """Kept set and order exactly the float64 oracle's (inputs re-drawn until no score lies within 1e-4 of the threshold and no centre
    within 1e-3 m of a limit - asserted here), z / vel bit-equal, x / y within 6 u E, score / dim / rot within the ulp bars."""
    H, W, nc = 9, 130, 2
    cfg = HH.DECODE_CFG_ALL if count == H * W else HH.DECODE_CFG
    raw, oracle = HH.decode_input(count, H, W, nc, 500 + count, cfg)
    assert oracle["margin_score"] > 1e-4 and oracle["margin_range"] > 1e-3 and len(oracle["pixel"]) == count
    measured, bars = HH.transcendental_bars(raw, nc)
    print("torch CPU fp32 vs float64, ulps:", measured, "device bars:", bars)
    got = _decode(raw[None], nc, cfg)
    _check_decoded(got, 0, oracle, bars, H, W, cfg, "count %d" % count)


def test_decode_capacity_smaller_than_the_count():
    H, W, nc = 9, 130, 2
    raw, oracle = HH.decode_input(257, H, W, nc, 757, HH.DECODE_CFG)
    _, bars = HH.transcendental_bars(raw, nc)
    got = _decode(raw[None], nc, HH.DECODE_CFG, cap=100)
    assert got["box"].shape == (1, 100, 9)
    _check_decoded(got, 0, oracle, bars, H, W, HH.DECODE_CFG, "cap 100 of 257", cap=100)


def test_decode_batch_with_an_empty_sample_in_the_middle_and_class_ties():
    H, W = 9, 130
    cases = [HH.decode_input(n, H, W, 2, 900 + n, HH.DECODE_CFG) for n in (65, 0, 257)]
    raw = torch.stack([c[0] for c in cases])
    # sample 0: two pixels whose two classes have the same logit: the first class wins
    tied = cases[0][1]["pixel"][:2]
    raw[0, 11].view(-1)[tied] = raw[0, 10].view(-1)[tied]
    oracles = [HH.decode_oracle(raw[b], 2, HH.DECODE_CFG) for b in range(3)]
    assert [len(o["pixel"]) for o in oracles] == [65, 0, 257] and oracles[0]["label"][:2].tolist() == [0, 0]
    assert all(o["margin_score"] > 1e-4 and o["margin_range"] > 1e-3 for o in oracles)
    _, bars = HH.transcendental_bars(raw, 2)
    got = _decode(raw, 2, HH.DECODE_CFG)
    again = _decode(raw, 2, HH.DECODE_CFG)
    for b in range(3):
        _check_decoded(got, b, oracles[b], bars, H, W, HH.DECODE_CFG, "sample %d" % b)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"


# a 257 x 256 map of 0.6 m pixels: every row inside in y, the border columns outside in x
DECODE_CFG_TALL = dict(HH.DECODE_CFG, post_center_limit_range=[-37.0, -3.0, -5.0, 113.0, 152.0, 3.0])


def test_decode_second_trip_of_the_block_count_scan():
    """257 x 256 pixels = exactly 257 blocks per image: the scan of an image's block counts makes a second trip of its carry loop, which
    holds one block.  Image 0 keeps pixels in the first block, in the last block of the first trip and in the block of the second;
    image 1 has another count, so a carry that survived from image 0 would show."""
    H, W, nc = 257, 256, 2
    assert H * W == 257 * 256
    cases = [HH.decode_input(n, H, W, nc, seed, DECODE_CFG_TALL) for n, seed in ((3000, 1257), (300, 2391))]
    raw = torch.stack([c[0] for c in cases])
    oracles = [c[1] for c in cases]
    assert all(o["margin_score"] > 1e-4 and o["margin_range"] > 1e-3 for o in oracles)
    blocks = (oracles[0]["pixel"] // 256).tolist()
    assert 0 in blocks and 255 in blocks and 256 in blocks and blocks[-1] == 256 and int(oracles[0]["pixel"][-1]) >= 65536
    assert [len(o["pixel"]) for o in oracles] == [3000, 300]  # (the counts differ: the carry starts at 0 for every image)
    _, bars = HH.transcendental_bars(raw, nc)
    got = _decode(raw, nc, DECODE_CFG_TALL)
    again = _decode(raw, nc, DECODE_CFG_TALL)
    for b in range(2):
        _check_decoded(got, b, oracles[b], bars, H, W, DECODE_CFG_TALL, "image %d" % b)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"


# ---- batched NMS ------------------------------------------------------------------------------------------------------

def _segments(sizes, seed):
    rng = np.random.default_rng(seed)
    segs = []
    for n in sizes:
        b = np.zeros((n, 7), np.float32)
        spread = max(2.0, 0.9 * np.sqrt(n))
        b[:, :2] = rng.uniform(-spread, spread, (n, 2))
        b[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, n)
        segs.append(b)
    return segs


def _nms_batch(segs, thresh, max_boxes):
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    S = len(segs)
    allb = np.concatenate(segs + [np.zeros((1, 7), np.float32)])  # (a trailing row: the array is never empty)
    boxes = torch.from_numpy(allb).to(dev)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in segs])]), dtype=torch.int32, device=dev)
    keep = torch.full((S, max_boxes), -7, dtype=torch.int32, device=dev)
    num = torch.full((S,), -7, dtype=torch.int32, device=dev)
    ws_bytes = lib.shasta_nms_batch_workspace_bytes(S, max_boxes)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
    hip.check(lib.shasta_nms_rotated_batch_f32(hip.ptr(boxes), hip.ptr(offsets), S, max_boxes, thresh, hip.ptr(ws), ws_bytes, hip.ptr(keep), hip.ptr(num),
                                               hip.stream_ptr()), "shasta_nms_rotated_batch_f32")
    torch.cuda.synchronize()
    return keep.cpu(), num.cpu()


def test_batched_nms_equals_the_single_calls_bit_for_bit():
    from shasta_amd import nms
    from oracle import nms_oracle as O
    sizes, thresh = [64, 0, 1, 300, 65, 0], 0.2
    segs = _segments(sizes, 11)
    keep, num = _nms_batch(segs, thresh, 300)
    for s, b in enumerate(segs):
        single = nms._nms_sorted(torch.from_numpy(b).to(_dev()), thresh).cpu().tolist() if len(b) else []
        assert int(num[s]) == len(single) and keep[s, :len(single)].tolist() == single, "segment %d" % s
        assert bool((keep[s, len(single):] == -7).all()), "segment %d: written past its count" % s
        assert len(single) < len(b) or len(b) <= 1  # (the boxes do overlap: something is suppressed)
    iou = O.iou_matrix(segs[4])
    assert float(np.abs(iou[np.triu_indices(65, 1)] - thresh).min()) > 1e-6
    want, _ = O.nms_sorted(segs[4], thresh, iou)
    assert keep[4, :int(num[4])].tolist() == list(want)
    # a segment longer than max_boxes is cut to its first max_boxes rows
    keep2, num2 = _nms_batch(segs, thresh, 64)
    cut = nms._nms_sorted(torch.from_numpy(segs[3][:64]).to(_dev()), thresh).cpu().tolist()
    assert keep2[3, :int(num2[3])].tolist() == cut and keep2[0, :int(num2[0])].tolist() == keep[0, :int(num[0])].tolist()
