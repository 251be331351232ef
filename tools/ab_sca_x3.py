"""A/B of the SCA block in the split-bf16 mode (BEVR_PREC_BF16X3) at the benchmark geometry: forward + backward of
SpatialCrossAttn (S = 200, 6 views, D = 5, 64 x 176 features, B samples), the pinned keys on the split-mode tap kernels
(BEVR_TAP_X3=1, ops.attention_core(tap_pix=...)) against the earlier routing (BEVR_TAP_X3=0: every key sampled, projected
and sent through the region / cell kernels).  The two routes alternate in ONE process (the switch is read per call), HIP
events around each step, one warm-up step per route; medians with min and max.
--gather: the A/B of the split-mode gather forward instead -- both routes with BEVR_TAP_X3=1, the scattered keys' forward
on bevr_attn_gather_fwd_x3 (BEVR_GATHER_X3=1) against the region forward (BEVR_GATHER_X3=0, the parent's routing).
--slab: the A/B of the split-mode slab backward -- both routes with BEVR_TAP_X3=1 and BEVR_GATHER_X3=0 (the defaults' forward),
the scattered keys' query-side backward on bevr_attn_slab_bwd_q_x3 (BEVR_SLAB_X3=1) against the query-tile kernel
(BEVR_SLAB_X3=0, the parent's routing).
--drop P: the block in training mode with attention dropout at rate P -- both routes with BEVR_TAP_X3=1, the pinned keys
on the split-mode tap dropout kernels (BEVR_TAP_X3_DROP=1: bevr_attn_tap_*_x3_dropout beside the region dropout kernels on
the scattered keys) against the parent's routing (the switch unset: every key sampled, projected and sent through the
region dropout kernels).  Each step draws its own mask seed; the routes' work does not depend on it.
--slab-rows: the block at config 5's geometry (S = 400, 128 x 352 features) with BEVR_TAP_X3=1 and BEVR_GATHER_X3=1 on both
sides, the scattered keys' query-side backward on the row-band slab kernel bevr_attn_slab_bwd_q_x3_rows (BEVR_SLAB_X3=2)
against BEVR_SLAB_X3=1, which at this side is the query-tile kernel.

    B=8 ITERS=5 python tools/ab_sca_x3.py [--gather | --slab | --slab-rows | --drop P] [out.json]"""
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevrender_amd import _lib, ops  # noqa: E402
from bevrender_amd.model.SCA import SpatialCrossAttn  # noqa: E402
from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector  # noqa: E402

DEV = "cuda"


def ring_rig(V, img_w, img_h):
    """bench.py's rig: V cameras on a ring (yaw 360 v / V, pitch 0, 1.5 m up), fx = fy = 0.8 W."""
    R0 = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)
    T, K = [], []
    for v in range(V):
        a = 2 * math.pi * v / V
        Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        M = np.eye(4)
        M[:3, :3] = Rz @ R0
        M[:3, 3] = (0, 0, 1.5)
        T.append(M)
        K.append(np.array([[0.8 * img_w, 0, img_w / 2, 0], [0, 0.8 * img_w, img_h / 2, 0], [0, 0, 1, 0]]))
    return T, K


def main():
    B, iters = int(os.environ.get("B", "8")), max(5, int(os.environ.get("ITERS", "5")))
    S, D, V, C, h, img_w, img_h = 200, 5, 6, 64, 2, 704, 256
    if "--slab-rows" in sys.argv[1:]:      # config 5's geometry: BEV 400, 6 cameras 512 x 1408
        S, img_w, img_h = 400, 1408, 512
    Hi, Wi = img_h // 4, img_w // 4
    T, K = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: K}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    argv = sys.argv[1:]
    drop_p = 0.0
    if "--drop" in argv:
        k = argv.index("--drop")
        drop_p = float(argv[k + 1])
        del argv[k:k + 2]
    sca = SpatialCrossAttn({"X": 50, "Y": 50, "Z": 2}, proj, S, D, -1.0, C, h, 1, 1, 3, B, True, n_views=V,
                           attn_drop_rate=drop_p, precision=_lib.PREC_BF16X3)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for prm in sca.parameters():
            prm.copy_(torch.randn(prm.shape, generator=gen) * (0.3 if prm.dim() == 1 else 1.0 / math.sqrt(max(1, prm[0].numel()))))
    sca = sca.to(DEV)          # (a fresh module is in training mode: attn_drop_rate > 0 draws a mask per step)
    q = torch.randn(B, C, S, S, generator=gen).to(DEV).requires_grad_(True)
    x = torch.randn(B * V, C, Hi, Wi, generator=gen).to(DEV).requires_grad_(True)
    cot = torch.randn(B, C, S, S, generator=gen).to(DEV)
    argv = [a for a in argv if a not in ("--gather", "--slab", "--slab-rows")]
    if "--slab-rows" in sys.argv[1:]:
        on = {"BEVR_TAP_X3": "1", "BEVR_GATHER_X3": "1"}
        new, routes = "slab_x3_rows", (("slab_x3_rows", dict(on, BEVR_SLAB_X3="2")), ("parent_route", dict(on, BEVR_SLAB_X3="1")))
    elif drop_p > 0.0:
        # (the parent's route: the switch UNSET, as a process that never heard of it)
        new, routes = "tap_x3_drop", (("tap_x3_drop", {"BEVR_TAP_X3": "1", "BEVR_TAP_X3_DROP": "1"}),
                                      ("parent_route", {"BEVR_TAP_X3": "1", "BEVR_TAP_X3_DROP": None}))
    elif "--slab" in sys.argv[1:]:
        new, routes = "slab_x3", (("slab_x3", {"BEVR_TAP_X3": "1", "BEVR_GATHER_X3": "0", "BEVR_SLAB_X3": "1"}),
                                  ("parent_route", {"BEVR_TAP_X3": "1", "BEVR_GATHER_X3": "0", "BEVR_SLAB_X3": "0"}))
    elif "--gather" in sys.argv[1:]:
        new, routes = "gather_x3", (("gather_x3", {"BEVR_TAP_X3": "1", "BEVR_GATHER_X3": "1"}),
                                    ("parent_route", {"BEVR_TAP_X3": "1", "BEVR_GATHER_X3": "0"}))
    else:
        new, routes = "tap_x3", (("tap_x3", {"BEVR_TAP_X3": "1"}), ("parent_route", {"BEVR_TAP_X3": "0"}))
    times = {new: [], "parent_route": []}
    kernels = {}

    def step(tag, sw, record):
        for k_, v_ in sw.items():
            if v_ is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v_
        for t in list(sca.parameters()) + [q, x]:
            t.grad = None
        if record:
            ops.KERNEL_TIMER.start()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, _ = sca(q, x, torch.tensor(0), None, False)
        out.backward(cot)
        e1.record()
        torch.cuda.synchronize()
        if record:
            kernels[tag] = {k: round(v["ms"], 2) for k, v in ops.KERNEL_TIMER.stop().items()}
        return e0.elapsed_time(e1)

    for it in range(iters + 1):
        for tag, sw in routes:
            ms = step(tag, sw, False)
            if it > 0:
                times[tag].append(ms)
    for tag, sw in routes:       # one more step of each with per-kernel events
        step(tag, sw, True)
    res = {"what": "SCA block forward + backward, bf16x3, S=%d, 6 views, B=%d%s; routes alternating in one process"
                   % (S, B, ", training mode, attention dropout p=%g" % drop_p if drop_p > 0.0 else ""),
           "routes": {tag: sw for tag, sw in routes}, "iters": iters}
    for tag, v in times.items():
        res[tag] = {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1),
                    "all_ms": [round(t, 1) for t in v]}
    res["ratio_new_over_parent"] = round(res[new]["median_ms"] / res["parent_route"]["median_ms"], 3)
    res["kernels_ms_one_step"] = kernels
    res["max_memory_allocated_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)      # of the device's 288
    print(json.dumps(res, indent=1))
    if argv:
        with open(argv[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
