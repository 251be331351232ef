"""What an attention call launches and computes, case by case, for comparing two versions of the host code on ONE built
library (a refactor of bevrender_amd/ops.py must change neither).

    python tools/route_trace.py run OUT.pt [--tree DIR]      every case once: launch lists + outputs + gradients -> OUT.pt
    python tools/route_trace.py compare A1.pt A2.pt A3.pt B.pt REPORT.txt

`run` imports bevrender_amd from DIR (default: this checkout) -- with BEVRENDER_LIB set both trees load the same library --
and replaces ops.KERNEL_TIMER.run with a recorder: per launch (timer name, C function, tag, flops, nbytes, number of
positional arguments, the integer arguments).  Only ops.attention_core, the SCA module and the timer are used, so the same
file runs against an older tree.  `compare` takes three runs of the base tree and one of the other: the launch lists must be
equal everywhere; a tensor the three base runs agree on bit for bit must be bit-equal in the fourth, any other (float
atomics: the order of the additions varies) may differ from a base run by at most twice the base runs' own spread."""
import argparse
import os
import sys

import torch

DEV = "cuda"
SWITCHES = ("BEVR_GATHER", "BEVR_SLAB", "BEVR_KNORM", "BEVR_MERGE_TAP", "BEVR_TAP", "BEVR_TAP_X3", "BEVR_TAP_X3_DROP", "BEVR_FUSED_KV",
            "BEVR_CELL", "BEVR_BWDK_LIST")


def core_case(ops, prec, seed, S=16, D=3, N=None, h=2, c=16, V=2, B=1, g=1, split=None, source="kv", tap_source=None,
              drop=None, Hi=8, Wi=20, outside=False, concat=True):
    """One attention_core call, forward + backward.  Keys [0, split) scattered over the image; keys [split, N) -- with
    tap_source: moved off pixel (0, 0) by offsets inside the learned range (inside the tap grid; outside=True puts one of
    them far outside), cell-sorted; without: anywhere, cell-sorted.  Returns the output and every input's gradient."""
    gen = torch.Generator().manual_seed(seed)
    C, P = h * c, B * V
    Hk, Wk = S // 2, S * D
    N = Hk * Wk if N is None else N
    Wt = 2 * S * D - 1
    ins = dict(query=torch.randn(B, C, S, S, generator=gen), table=torch.randn(h, 2 * S - 1, Wt, generator=gen) * 0.3)
    pos = (torch.rand(P * g, N, 2, generator=gen) * 2 - 1) * 1.05
    if split is not None and split < N:
        tail = pos[:, split:]
        if tap_source:
            off = torch.tanh(torch.randn(P, N - split, 2, generator=gen) * 1.5)
            tail = off * torch.tensor([5.0 / (Hk - 1), 5.0 / (Wk - 1)]) - 1.0
            if outside:
                tail[0, (N - split) // 2] = 0.9
        if g == 1:
            a, b = ops.key_coords(tail, S, Wt, N - split)
            tail = tail.gather(1, ops.cell_order(a, b)[..., None].expand(-1, -1, 2))
        pos = torch.cat((pos[:, :split], tail), 1)
    ins["pos"] = pos
    if source == "kv":
        ins["kv"] = torch.randn(P, N, 2 * C, generator=gen)
    else:
        ins["feat"] = torch.randn(P, Hi, Wi, C, generator=gen)
        ins["Wkv"] = torch.randn(2 * C, C, generator=gen) * C ** -0.5
        ins["bkv"] = torch.randn(2 * C, generator=gen) * 0.3
        if source == "tap_pix":
            ins["kv"] = torch.randn(P, split, 2 * C, generator=gen)
    cot = torch.randn(B if concat else P, S * S, (V if concat else 1) * C, generator=gen)
    t = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}
    kw = dict(heads=h, groups=g, views=V, precision=prec, cell_split=split, tap_source=tap_source, attn_drop=drop,
              concat_views=concat, kv=t.get("kv"))
    if source != "kv":
        kw[source] = (t["feat"], t["Wkv"], t["bkv"])
    out = ops.attention_core(t["query"], None, None, t["pos"], t["table"], **kw)
    (out * cot.to(DEV)).sum().backward()
    res = {"out": out.detach()}
    res.update({"d_" + k: v.grad for k, v in t.items() if v.grad is not None})
    return res


def module_case(ops, prec, seed, train, drop_rate=0.4, S=32, D=3, h=2, C=64, V=2, B=2, Hi=8, Wi=20, cs=400, static_split=False):
    """SCADeformableAttention with the keys [cs, N) of every view pinned at (-1, -1), split_is_pinned=True; static_split:
    key order and split from ops.split_key_order (what SpatialCrossAttn passes) instead of cs."""
    from bevrender_amd.model.SCA_deform_attn import SCADeformableAttention
    torch.manual_seed(seed)
    Hk, Wk = S // 2, S * D
    N = Hk * Wk
    m = SCADeformableAttention(S, D, C, h, 1, 1, 3, True, B, n_views=V, attn_drop_rate=drop_rate, precision=prec)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.1 if p.ndim > 1 else 0.05))
    q, x = torch.randn(B, C, S, S), torch.randn(B, V, C, Hi, Wi)
    ref = torch.rand(1, V, N, 2) * 2.2 - 1.1
    ref[:, :, cs:] = -1.0
    kw = dict(cell_split=cs, split_is_pinned=True)
    if static_split:
        order, split = ops.split_key_order(ref[0][..., (1, 0)].numpy(), S, 2 * S * D - 1, min_cell_keys=64)
        kw = dict(key_order=order.to(DEV), cell_split=split if split < N else None, split_is_pinned=True)
    ref = ref.reshape(1, V, Hk, Wk, 2).expand(B, -1, -1, -1, -1).contiguous()
    cot = torch.randn(B, C, S, S)
    m = m.to(DEV).train(train)
    qg, xg = q.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    out, _ = m(xg, qg, ref.to(DEV), {}, False, **kw)
    (out * cot.to(DEV)).sum().backward()
    res = {"out": out.detach(), "d_query": qg.grad, "d_x": xg.grad}
    res.update({"d_" + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    return res


def cases(ops, _lib):
    F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16
    name = {F32: "f32", X3: "bf16x3", BF16: "bf16", F16: "f16"}
    out = []

    def add(label, fn, *a, env=None, **kw):
        out.append((label, env or {}, lambda: fn(ops, *a, **kw)))

    # the four routes of tests/test_gpu_random_sweep_routes.py, every precision each supports
    for i, p in enumerate((F32, X3, BF16, F16)):
        add(f"kv_cell-{name[p]}", core_case, p, 10 + i, N=200, split=72)
    for i, p in enumerate((F32, X3, BF16, F16)):
        add(f"kv_region-{name[p]}", core_case, p, 20 + i, N=200)
    add("kv_region-bf16-tsa_table", core_case, BF16, 24, D=1, N=200)
    for i, p in enumerate((BF16, F16)):
        add(f"kv_source-{name[p]}", core_case, p, 30 + i, N=200, split=72, source="kv_source")
        add(f"kv_source-region-{name[p]}", core_case, p, 32 + i, N=200, source="kv_source", concat=False)
        add(f"tap-{name[p]}", core_case, p, 40 + i, split=130, source="kv_source", tap_source=True)
        add(f"tap-only-{name[p]}", core_case, p, 42 + i, split=0, source="kv_source", tap_source=True)
    # dropout against tap_source, the checked keys inside the tap grid and one of them outside it
    for ts in (False, True, "pinned"):
        for outside in (False, True):
            if ts == "pinned" and outside:
                continue        # a broken promise: not a case
            add(f"dropout-tap_source={ts}-{'outside' if outside else 'inside'}", core_case, BF16, 50, split=130,
                source="kv_source", tap_source=ts if ts else None, drop=(0.3, 1234), outside=outside)
    add("dropout-kv-f32", core_case, F32, 51, N=200, split=72, drop=(0.3, 99))
    add("dropout-kv_source-f16", core_case, F16, 52, N=200, source="kv_source", drop=(0.5, 7))
    add("tap_pix-bf16x3", core_case, X3, 60, split=130, source="tap_pix", tap_source="pinned", env={"BEVR_TAP_X3": "1"})
    add("gather-bands-f16-S400", core_case, F16, 61, S=400, D=1, N=96, h=1, c=8, V=1)
    add("kv_source-groups2", core_case, BF16, 62, N=200, g=2, source="kv_source")
    add("kv_source-groups2-dropout", core_case, BF16, 63, N=200, g=2, source="kv_source", drop=(0.2, 5))
    for train in (True, False):
        add(f"sca-module-bf16-{'train' if train else 'eval'}", module_case, BF16, 70, train)
    add("sca-module-f32-train", module_case, F32, 71, True)
    add("sca-module-bf16x3-eval", module_case, X3, 72, False)
    add("sca-module-bf16x3-eval-tap_x3", module_case, X3, 72, False, env={"BEVR_TAP_X3": "1"})
    add("sca-module-bf16x3-train-tap_x3", module_case, X3, 73, True, env={"BEVR_TAP_X3": "1"})
    # the A/B switches, one at a time
    add("BEVR_GATHER=0", core_case, BF16, 80, N=200, env={"BEVR_GATHER": "0"})
    add("BEVR_SLAB=0", core_case, BF16, 81, N=200, env={"BEVR_SLAB": "0"})
    add("BEVR_SLAB=2", core_case, BF16, 82, D=1, N=200, env={"BEVR_SLAB": "2"})
    add("BEVR_TAP=0", module_case, BF16, 83, False, env={"BEVR_TAP": "0"})
    add("BEVR_KNORM=0", core_case, BF16, 84, N=200, source="kv_source", env={"BEVR_KNORM": "0"})
    add("BEVR_MERGE_TAP=0", core_case, BF16, 85, split=130, source="kv_source", tap_source=True, env={"BEVR_MERGE_TAP": "0"})
    add("BEVR_FUSED_KV=0", module_case, BF16, 86, False, env={"BEVR_FUSED_KV": "0"})
    add("BEVR_CELL=1-static-split", module_case, BF16, 87, False, static_split=True)
    add("BEVR_CELL=0", module_case, BF16, 87, False, static_split=True, env={"BEVR_CELL": "0"})
    return out


def run(out_path, tree):
    sys.path.insert(0, os.path.abspath(tree))
    from bevrender_amd import _lib, ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree)), ops.__file__
    launches = []

    def recorder(name, flops, fn, *args, nbytes=0.0, tag=""):
        ints = [a for a in args if isinstance(a, int) and not isinstance(a, bool)]
        launches.append((name, getattr(fn, "__name__", repr(fn)), tag, float(flops), float(nbytes), len(args), ints))
        return fn(*args)
    ops.KERNEL_TIMER.run = recorder
    result = {}
    for label, env, fn in cases(ops, _lib):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        del launches[:]
        tensors = fn()
        torch.cuda.synchronize()
        result[label] = {"launches": list(launches), "tensors": {k: v.detach().float().cpu() for k, v in tensors.items()}}
        print(f"{label}: {len(launches)} timed launches, {len(tensors)} tensors", flush=True)
    torch.save(result, out_path)


def _diff(a, b):
    if a.shape != b.shape:
        return float("inf")
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return 0.0 if bool(same.all()) else float((a - b).abs()[~same].max())


def compare(base_paths, other_path, report):
    base = [torch.load(p) for p in base_paths]
    other = torch.load(other_path)
    lines, bad = [], 0
    assert list(other) == list(base[0]), "the case lists differ"
    for label in base[0]:
        lists = [r[label]["launches"] for r in base]
        stable = all(l == lists[0] for l in lists[1:])
        equal = other[label]["launches"] == lists[0]
        worst = []
        ok = stable and equal
        assert set(other[label]["tensors"]) == set(base[0][label]["tensors"]), label
        for k in base[0][label]["tensors"]:
            ts = [r[label]["tensors"][k] for r in base]
            spread = max(_diff(ts[i], ts[j]) for i in range(3) for j in range(i))
            d = max(_diff(other[label]["tensors"][k], t) for t in ts)
            good = d == 0.0 if spread == 0.0 else d <= 2.0 * spread
            ok &= good
            if spread > 0.0 or not good:
                worst.append(f"{k}: spread {spread:.3e} diff {d:.3e}{'' if good else ' FAIL'}")
        bad += not ok
        lines.append(f"{label}: {len(lists[0])} launches, lists {'equal' if equal else 'DIFFER'}"
                     f"{'' if stable else ' (base runs DIFFER among themselves)'}; "
                     f"{len(base[0][label]['tensors'])} tensors, "
                     + ("all bit-equal" if not worst else "not bit-stable in the base runs: " + "; ".join(worst))
                     + f" -> {'ok' if ok else 'FAIL'}")
        if not equal:
            for i, (x, y) in enumerate(zip(lists[0], other[label]["launches"])):
                if x != y:
                    lines.append(f"    first difference at launch {i}: {x} != {y}")
                    break
            else:
                lines.append(f"    lengths {len(lists[0])} != {len(other[label]['launches'])}")
    lines.append(f"{len(base[0])} cases, {bad} failed")
    with open(report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "compare"))
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if a.mode == "run":
        run(a.paths[0], a.tree)
    else:
        sys.exit(1 if compare(a.paths[:3], a.paths[3], a.paths[4]) else 0)
