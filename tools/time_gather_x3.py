"""Per-launch time of the split-bf16 gather forward (bevr_attn_gather_fwd_x3, BEVR_GATHER_X3=1) against the region forward
it replaces (bevr_attn_fwd in BEVR_PREC_BF16X3) on the same inputs, at the two launch shapes of the benchmark:
  SCA: S = 200, D = 5 (table 399 x 1999), the ~36 000 scattered keys of a view in k-d order, 2 heads x 12 problems
  TSA: S = 200, table 399 x 399, 40 000 grid keys in k-d order, 2 heads x 8 problems
HIP events around each launch (ops.KERNEL_TIMER), one warm-up call per route, then rounds of 7 calls per route in both
orders; per route and order the median with min and max.  The outputs of the two routes are compared at the timed size.

    python tools/time_gather_x3.py [out.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevrender_amd import _lib, ops  # noqa: E402

DEV = "cuda"
ROUTES = {"gather_x3": ("1", "bevr_attn_gather_fwd"), "region": ("0", "bevr_attn_fwd")}      # switch, timer name


def inputs(kind, gen):
    S, C, h = 200, 64, 2
    if kind == "SCA":
        D, N, B, V = 5, 36000, 2, 6
        base = (torch.rand(1, N, 2, generator=gen) * 2 - 1) * 0.95
        jitter = 0.01
    else:
        D, B, V = 1, 8, 1
        g = (torch.arange(S, dtype=torch.float32) + 0.5) / S * 2 - 1
        base = torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(1, S * S, 2)
        N, jitter = S * S, 0.5 / (S - 1)
    Wt = 2 * S * D - 1
    order = torch.from_numpy(ops.kd_key_order(base[0].double().numpy(), S, Wt))
    pos = base[:, order] + (torch.rand(B * V, N, 2, generator=gen) * 2 - 1) * jitter
    query = torch.randn(B, C, S, S, generator=gen)
    k = torch.randn(B * V, N, C, generator=gen)
    v = torch.randn(B * V, N, C, generator=gen)
    table = torch.randn(h, 2 * S - 1, Wt, generator=gen) * 0.3
    return [t.to(DEV) for t in (query, k, v, pos, table)], h, V, N, B * V


def call(ins, h, V, route):
    sw, timer = ROUTES[route]
    os.environ["BEVR_GATHER_X3"] = sw
    ops.KERNEL_TIMER.start()
    with torch.no_grad():
        out = ops.attention_core(*ins, heads=h, groups=1, views=V, precision=_lib.PREC_BF16X3)
    rec = ops.KERNEL_TIMER.stop()
    assert timer in rec and rec[timer]["n"] == 1, sorted(rec)
    assert ("bevr_attn_fwd" in rec) == (route == "region"), sorted(rec)
    return rec[timer]["ms"], out


def main():
    gen = torch.Generator().manual_seed(13)
    lines = []
    for kind in ("SCA", "TSA"):
        ins, h, V, N, n_prob = inputs(kind, gen)
        outs = {r: call(ins, h, V, r)[1] for r in ROUTES}          # warm-up, and the outputs
        e = (outs["gather_x3"] - outs["region"]).abs().max().item() / outs["region"].abs().max().item()
        lines.append(f"{kind}: S=200 N={N} problems={n_prob} heads={h}; gather_x3 against region output: {e:.3e}")
        for first, second in (("gather_x3", "region"), ("region", "gather_x3")):
            ms = {first: [], second: []}
            for _ in range(7):
                for r in (first, second):
                    ms[r].append(call(ins, h, V, r)[0])
            med = {r: statistics.median(v) for r, v in ms.items()}
            for r in (first, second):
                lines.append(f"{kind} order {first} first: {r:9s} median {med[r]:8.2f} ms  min {min(ms[r]):8.2f}  max {max(ms[r]):8.2f}")
            lines.append(f"{kind} order {first} first: gather_x3 / region = {med['gather_x3'] / med['region']:.3f}")
        del ins, outs
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
