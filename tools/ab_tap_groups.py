"""A/B of the SCA block with TWO channel groups at the benchmark geometry: forward + backward of SpatialCrossAttn
(S = 200, 6 views, D = 5, 64 x 176 features, bf16 operands, n_groups = 2, B samples), the pinned keys on the two-group
tap kernels (BEVR_TAP_GROUPS=1: csrc/attn_tap_*_g2.hip, every (problem, group) in its own cell order) against the
parent's route (the switch UNSET: the split dropped, every key sampled, projected and sent through the gather forward
and the slab / region backward).  The two routes alternate in ONE process (the switch is read per call), HIP events
around each step, two warm-up steps per route; median, minimum and maximum per route, the outputs and the query
gradient of the two routes compared on the way, and one more step of each with per-kernel events.

    B=2 ITERS=7 python tools/ab_tap_groups.py [out.txt]"""
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bevrender_amd import _lib, ops  # noqa: E402
from bevrender_amd.model.SCA import SpatialCrossAttn  # noqa: E402
from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector  # noqa: E402
from ab_sca_x3 import ring_rig  # noqa: E402

DEV = "cuda"
WARMUP = 2


def main():
    B, iters = int(os.environ.get("B", "2")), max(5, int(os.environ.get("ITERS", "7")))
    S, D, V, C, h, img_w, img_h = 200, 5, 6, 64, 2, 704, 256
    Hi, Wi = img_h // 4, img_w // 4
    T, K = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: K}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    sca = SpatialCrossAttn({"X": 50, "Y": 50, "Z": 2}, proj, S, D, -1.0, C, h, 2, 1, 3, B, True, n_views=V,
                           precision=_lib.PREC_BF16)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for prm in sca.parameters():
            prm.copy_(torch.randn(prm.shape, generator=gen) * (0.3 if prm.dim() == 1 else 1.0 / math.sqrt(max(1, prm[0].numel()))))
    sca = sca.to(DEV)
    q = torch.randn(B, C, S, S, generator=gen).to(DEV).requires_grad_(True)
    x = torch.randn(B * V, C, Hi, Wi, generator=gen).to(DEV).requires_grad_(True)
    cot = torch.randn(B, C, S, S, generator=gen).to(DEV)
    routes = (("tap_groups", {"BEVR_TAP_GROUPS": "1"}), ("parent_route", {"BEVR_TAP_GROUPS": None}))
    times = {tag: [] for tag, _ in routes}
    kernels, last = {}, {}

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
        last[tag] = (out.detach().float().clone(), q.grad.detach().float().clone())
        return e0.elapsed_time(e1)

    for it in range(iters + WARMUP):
        for tag, sw in routes:
            ms = step(tag, sw, False)
            if it >= WARMUP:
                times[tag].append(ms)
    for tag, sw in routes:       # one more step of each with per-kernel events
        step(tag, sw, True)

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    res = {"what": "SCA block forward + backward, bf16, n_groups=2, S=200, D=5, 6 views, 64 x 176 features, B=%d; routes "
                   "alternating in one process after %d warm-up steps each, HIP events around every step" % (B, WARMUP),
           "routes": {tag: sw for tag, sw in routes}, "iters": iters}
    for tag, v in times.items():
        res[tag] = {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1),
                    "all_ms": [round(t, 1) for t in v]}
    res["ratio_new_over_parent_median"] = round(res["tap_groups"]["median_ms"] / res["parent_route"]["median_ms"], 3)
    res["routes_agree"] = {"out_rel": float("%.3g" % rel(last["tap_groups"][0], last["parent_route"][0])),
                           "dquery_rel": float("%.3g" % rel(last["tap_groups"][1], last["parent_route"][1]))}
    res["kernels_ms_one_step"] = kernels
    text = json.dumps(res, indent=1)
    print(text)
    if sys.argv[1:]:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
