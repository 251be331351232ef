"""Timing of attention dropout on the gather forward and the slab bwd_q (BEVR_SCATTER_DROP=1, bf16, p = 0.1).

Per kernel: ops.attention_core on a scattered key segment of the benchmark's size (S = 200, D = 5, 12 problems x 2 heads,
N = 36 000 keys in the static k-d order), forward + backward, per-kernel HIP events (ops.KERNEL_TIMER), medians of 7:
each new kernel against the region dropout kernel it replaces (the switch unset) and against its own no-mask version (the
same call without attn_drop).

Per block: forward + backward of SpatialCrossAttn at the benchmark geometry (S = 200, 6 views, D = 5, 64 x 176 features,
B samples) in training mode with attn_drop_rate = 0.1, this route (BEVR_SCATTER_DROP=1) and the parent commit's route (the
switch UNSET: the scattered keys on the region dropout kernels) alternating in ONE process, HIP events around each step,
one warm-up step per route; medians of 5 with min and max, and the per-kernel times of one more step of each.

--x3: the same two measurements in the split-bf16 mode (bf16x3), where the switch moves the scattered keys' bwd_q alone
(bevr_attn_slab_bwd_q_x3_dropout against bevr_attn_bwd_q_dropout, and against its no-mask version bevr_attn_slab_bwd_q_x3,
which runs under the slab route's timer name).  Every route of that mode runs with BEVR_TAP_X3=1 BEVR_TAP_X3_DROP=1
BEVR_SLAB_X3=1; BEVR_SCATTER_DROP is the one difference.  --kernel-only: the per-kernel part alone.

    B=8 python tools/ab_scatter_drop.py [--x3] [--kernel-only] [out.json]"""
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_sca_x3 import ring_rig  # noqa: E402
from bevrender_amd import _lib, ops  # noqa: E402
from bevrender_amd.model.SCA import SpatialCrossAttn  # noqa: E402
from bevrender_amd.model.bev_cmr_proj import BEV2CameraProjector  # noqa: E402

DEV = "cuda"
P = 0.1
ROUTES = (("scatter_drop", {"BEVR_SCATTER_DROP": "1"}, True), ("region_drop", {"BEVR_SCATTER_DROP": None}, True),
          ("no_mask", {"BEVR_SCATTER_DROP": None}, False))
K = ops.K
PAIRS = {"forward": {"scatter_drop": K.GATHER_DROP, "region_drop": K.FWD_DROP, "no_mask": K.GATHER},
         "bwd_q": {"scatter_drop": K.SLAB_BWD_Q_DROP, "region_drop": K.BWD_Q_DROP, "no_mask": K.SLAB_BWD_Q}}
# the split-bf16 mode: its switches on every route; the no-mask slab kernel is timed under the slab route's name
X3_BASE = {"BEVR_TAP_X3": "1", "BEVR_TAP_X3_DROP": "1", "BEVR_SLAB_X3": "1"}
X3_PAIRS = {"bwd_q": {"scatter_drop": K.SLAB_BWD_Q_X3_DROP, "region_drop": K.BWD_Q_DROP, "no_mask": K.SLAB_BWD_Q}}


def switches(sw):
    for k_, v_ in sw.items():
        if v_ is None:
            os.environ.pop(k_, None)
        else:
            os.environ[k_] = v_


def stats(v):
    return {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}


def per_kernel(iters=7, x3=False):
    prec, pairs = (_lib.PREC_BF16X3, X3_PAIRS) if x3 else (_lib.PREC_BF16, PAIRS)
    S, D, C, h, n_prob, N = 200, 5, 64, 2, 12, 36000
    Wt = 2 * S * D - 1
    gen = torch.Generator().manual_seed(5)
    pos = (torch.rand(1, N, 2, generator=gen) * 2 - 1) * 0.95
    order = torch.from_numpy(ops.kd_key_order(pos[0].double().numpy(), S, Wt))
    pos = pos[:, order].expand(n_prob, -1, -1).contiguous().to(DEV)
    query = torch.randn(n_prob, C, S, S, generator=gen).to(DEV).requires_grad_(True)
    kv = torch.randn(n_prob, N, 2 * C, generator=gen).to(DEV).requires_grad_(True)
    table = (torch.randn(h, 2 * S - 1, Wt, generator=gen) * 0.3).to(DEV).requires_grad_(True)
    cot = torch.randn(n_prob, S * S, C, generator=gen).to(DEV)
    ms = {tag: {} for tag, _, _ in ROUTES}
    for it in range(iters + 1):
        for tag, sw, drop in ROUTES:
            switches(dict(X3_BASE, **sw) if x3 else sw)
            for t in (query, kv, table):
                t.grad = None
            ops.KERNEL_TIMER.start()
            out = ops.attention_core(query, None, None, pos, table, heads=h, groups=1, views=1, precision=prec,
                                     kv=kv, attn_drop=(P, 1000 + it) if drop else None)
            out.backward(cot)
            rec = ops.KERNEL_TIMER.stop()
            if it > 0:
                for k_, v_ in rec.items():
                    ms[tag].setdefault(k_, []).append(v_["ms"])
    res = {"what": "scattered segment alone: S=200, D=5, %d problems x %d heads, N=%d, %s, p=%g; per-kernel HIP events, "
                   "medians of %d" % (n_prob, h, N, "bf16x3" if x3 else "bf16", P, iters)}
    for what, names in pairs.items():
        row = {tag: dict(kernel=name, **stats(ms[tag][name])) for tag, name in names.items()}
        row["new_over_region_dropout"] = round(row["scatter_drop"]["median_ms"] / row["region_drop"]["median_ms"], 3)
        row["new_over_no_mask"] = round(row["scatter_drop"]["median_ms"] / row["no_mask"]["median_ms"], 3)
        res[what] = row
    return res


def per_block(B, iters=5, x3=False):
    S, D, V, C, h, img_w, img_h = 200, 5, 6, 64, 2, 704, 256
    Hi, Wi = img_h // 4, img_w // 4
    T, Kc = ring_rig(V, img_w, img_h)
    proj = BEV2CameraProjector(imu_to_rgb={0: T}, K={0: Kc}, vehicle_type_code=0, img_width=img_w, img_height=img_h,
                               ori_img_width=img_w, ori_img_height=img_h, device=DEV)
    sca = SpatialCrossAttn({"X": 50, "Y": 50, "Z": 2}, proj, S, D, -1.0, C, h, 1, 1, 3, B, True, n_views=V,
                           attn_drop_rate=P, precision=_lib.PREC_BF16X3 if x3 else _lib.PREC_BF16)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for prm in sca.parameters():
            prm.copy_(torch.randn(prm.shape, generator=gen) * (0.3 if prm.dim() == 1 else 1.0 / math.sqrt(max(1, prm[0].numel()))))
    sca = sca.to(DEV)          # (a fresh module is in training mode: a mask per step)
    q = torch.randn(B, C, S, S, generator=gen).to(DEV).requires_grad_(True)
    x = torch.randn(B * V, C, Hi, Wi, generator=gen).to(DEV).requires_grad_(True)
    cot = torch.randn(B, C, S, S, generator=gen).to(DEV)
    routes = (("scatter_drop", {"BEVR_SCATTER_DROP": "1"}), ("parent_route", {"BEVR_SCATTER_DROP": None}))
    if x3:
        routes = tuple((tag, dict(X3_BASE, **sw)) for tag, sw in routes)
    times, kernels = {tag: [] for tag, _ in routes}, {}

    def step(tag, sw, record):
        switches(sw)
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
            kernels[tag] = {k_: round(v_["ms"], 2) for k_, v_ in ops.KERNEL_TIMER.stop().items()}
        return e0.elapsed_time(e1)

    for it in range(iters + 1):
        for tag, sw in routes:
            t_ms = step(tag, sw, False)
            if it > 0:
                times[tag].append(t_ms)
    for tag, sw in routes:
        step(tag, sw, True)
    res = {"what": "SCA block forward + backward, %s, S=200, 6 views, B=%d, training mode, attention dropout p=%g; routes "
                   "alternating in one process, medians of %d" % ("bf16x3" if x3 else "bf16", B, P, iters),
           "routes": {tag: sw for tag, sw in routes}}
    for tag, v in times.items():
        res[tag] = dict(stats(v), all_ms=[round(t, 1) for t in v])
    res["ratio_new_over_parent"] = round(res["scatter_drop"]["median_ms"] / res["parent_route"]["median_ms"], 3)
    res["kernels_ms_one_step"] = kernels
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    x3 = "--x3" in sys.argv
    res = {"per_kernel": per_kernel(x3=x3)}
    if "--kernel-only" not in sys.argv:
        res["per_block"] = per_block(int(os.environ.get("B", "8")), x3=x3)
    print(json.dumps(res, indent=1))
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
