"""Per-launch time of the split-bf16 slab query-side backward (bevr_attn_slab_bwd_q_x3, BEVR_SLAB_X3=1) against the
query-tile kernel it replaces (bevr_attn_bwd_q in BEVR_PREC_BF16X3) on the same inputs, at the SCA launch shape of the
benchmark: S = 200, D = 5 (table 399 x 1999), the ~36 000 scattered keys of a view in k-d order, 2 heads x 12 problems.
HIP events around each launch (ops.KERNEL_TIMER) inside a forward + backward of ops.attention_core, one warm-up call per
route, then rounds of 7 calls per route in both orders; per route and order the median with min and max.  The query and
table gradients of the two routes are compared at the timed size.

--bev S: another BEV side.  Above 211 the slab route is the row-band kernel (bevr_attn_slab_bwd_q_x3_rows, BEVR_SLAB_X3=2)
and a figure is the SUM of a call's band launches (ops.slab_bands(S)); --keys, --batch and --views size the launch
(config 5, S = 400: about 144 000 scattered keys per view).

    python tools/time_slab_x3.py [out.txt] [--bev S --keys N --batch B --views V]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevrender_amd import _lib, ops  # noqa: E402

DEV = "cuda"
ROUTES = {"slab_x3": ("1", "bevr_attn_slab_bwd_q"), "tile": ("0", "bevr_attn_bwd_q")}      # switch, timer name


def inputs(gen, S=200, N=36000, B=2, V=6):
    C, h, D = 64, 2, 5
    Wt = 2 * S * D - 1
    base = (torch.rand(1, N, 2, generator=gen) * 2 - 1) * 0.95
    order = torch.from_numpy(ops.kd_key_order(base[0].double().numpy(), S, Wt))
    pos = base[:, order] + (torch.rand(B * V, N, 2, generator=gen) * 2 - 1) * 0.01
    query = torch.randn(B, C, S, S, generator=gen)
    k = torch.randn(B * V, N, C, generator=gen)
    v = torch.randn(B * V, N, C, generator=gen)
    table = torch.randn(h, 2 * S - 1, Wt, generator=gen) * 0.3
    cot = torch.randn(B * V, S * S, C, generator=gen)
    return [t.to(DEV) for t in (query, k, v, pos, table)], cot.to(DEV), h, V, N, B * V


def call(ins, cot, h, V, route, launches=1):
    sw, timer = ROUTES[route]
    os.environ["BEVR_SLAB_X3"] = sw
    leaves = [t.detach().requires_grad_(i in (0, 4)) for i, t in enumerate(ins)]      # the query-side gradients alone
    ops.KERNEL_TIMER.start()
    out = ops.attention_core(*leaves, heads=h, groups=1, views=V, precision=_lib.PREC_BF16X3)
    out.backward(cot)
    rec = ops.KERNEL_TIMER.stop()
    assert timer in rec and rec[timer]["n"] == (launches if route == "slab_x3" else 1), sorted(rec)
    assert ("bevr_attn_bwd_q" in rec) == (route == "tile"), sorted(rec)
    return rec[timer]["ms"], leaves[0].grad, leaves[4].grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--bev", type=int, default=200)
    ap.add_argument("--keys", type=int, default=36000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--views", type=int, default=6)
    a = ap.parse_args()
    S = a.bev
    launches = 1
    if S > 211:      # the row-band kernel: the switch's value 2, one launch per band
        ROUTES["slab_x3"] = ("2", "bevr_attn_slab_bwd_q")
        launches = len(ops.slab_bands(S))
    gen = torch.Generator().manual_seed(13)
    lines = []
    ins, cot, h, V, N, n_prob = inputs(gen, S, a.keys, a.batch, a.views)
    g = {r: call(ins, cot, h, V, r, launches)[1:] for r in ROUTES}          # warm-up, and the gradients
    eq = (g["slab_x3"][0] - g["tile"][0]).abs().max().item() / g["tile"][0].abs().max().item()
    et = (g["slab_x3"][1] - g["tile"][1]).abs().max().item() / g["tile"][1].abs().max().item()
    lines.append(f"SCA: S={S} N={N} problems={n_prob} heads={h} slab launches per call={launches}; slab_x3 against "
                 f"query-tile: dQ {eq:.3e} d(table) {et:.3e}")
    del g
    for first, second in (("slab_x3", "tile"), ("tile", "slab_x3")):
        ms = {first: [], second: []}
        for _ in range(7):
            for r in (first, second):
                ms[r].append(call(ins, cot, h, V, r, launches)[0])
        med = {r: statistics.median(v) for r, v in ms.items()}
        for r in (first, second):
            lines.append(f"SCA order {first} first: {r:8s} median {med[r]:8.2f} ms  min {min(ms[r]):8.2f}  max {max(ms[r]):8.2f}")
        lines.append(f"SCA order {first} first: slab_x3 / tile = {med['slab_x3'] / med['tile']:.3f}")
    lines.append(f"SCA: max memory allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
