"""Seeded random sweep of attention DROPOUT (bevr_attn_fwd_dropout / _bwd_q_dropout / _bwd_k_dropout) against one
float64 oracle per configuration: explicit K | V in every mode and the fused K | V source in the 16-bit modes, channel
groups, N across the key-side kernel's 384-key workgroup, all four key-position kinds, concat_views, and rates from a
few 2^-16 up to 0.5.  cell_split / tap_source are passed at random: with dropout they are ignored.  The oracle's mask
is the host twin of the kernels' (ops.dropout_keep_mask, in the caller's key order) times 1 / (1 - p).  Forward and
every input's gradient against the limits of tests/test_gpu_random_sweep_routes.py; each case asserts that the three
dropout kernels ran and no other attention kernel did, and that another seed changes the output exactly when it
changes the mask.  BEVR_SWEEP=n widens it (n configurations per mode)."""
import os

import numpy as np
import pytest
import torch

from bevrender_amd import _lib, ops
from test_gpu_dropout import _oracle_core_drop, drop_mult
from test_gpu_fullsize import kink_distance
from test_gpu_ops import GRAD_LIM, rel_err
from test_gpu_random_sweep_routes import (MODE_NAME, OUT_LIM, POS_LIM, UNIT, chain_kv, gradient_terms, make,
                                          pixel_kink_distance)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NSEED = int(os.environ.get("BEVR_SWEEP", "16"))
F32, X3, BF16, F16 = _lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16, _lib.PREC_F16

DROP_MODES = [("kv", p) for p in (F32, X3, BF16, F16)] + [("kv_source", p) for p in (BF16, F16)]
DROP_KERNELS = ("bevr_attn_fwd_dropout", "bevr_attn_bwd_q_dropout", "bevr_attn_bwd_k_dropout")
OTHER_ATTN = ("bevr_attn_fwd", "bevr_attn_bwd_q", "bevr_attn_bwd_k", "bevr_attn_gather_fwd", "bevr_attn_slab_bwd_q",
              "bevr_attn_cell_fwd", "bevr_attn_cell_bwd_q", "bevr_attn_cell_bwd_k", "bevr_attn_tap_fwd",
              "bevr_attn_tap_bwd_q", "bevr_attn_tap_bwd_k")
# a few 2^-16 (the threshold's first steps: nearly every pair kept) and the rates the reference trains with
RATES = [1 / 65536, 3 / 65536, 17 / 65536, 0.1, 0.3, 0.5]


def draw_drop(route, prec, seed):
    """One configuration: the routes sweep's shape distribution (S, D, N, h, c, V, B, key kinds), groups 1 / 2 / 4, a
    random cell_split / tap_source that dropout must ignore, and a rate."""
    for t in range(1000):
        r = np.random.RandomState(10007 * seed + 131 * prec + (0 if route == "kv" else 1) + 7919 * t + 555)
        h = int(r.choice([1, 2, 4]))
        c = int(r.choice([8, 16, 32]))
        V = int(r.choice([1, 1, 2, 3]))
        B = int(r.choice([1, 2]))
        S = int(r.choice([3, 5, 8, 13, 17, 21, 31, 32, 33, 40]))
        D = int(r.choice([1, 2, 3, 5, 9]))
        N = int(r.choice([7, 31, 32, 33, 63, 64, 65, 127, 200, 383, 384, 385, 450]))
        g = int(r.choice([d for d in (1, 2, 4) if h % d == 0]))
        # what the caller passes: dropout keeps every key on the region kernels whatever it says
        split = [None, 0, int(r.randint(0, N + 1)), N][r.randint(0, 4)]
        cfg = dict(route=route, prec=prec, h=h, C=h * c, V=V, B=B, S=S, D=D, N=N, g=g, kind=int(r.randint(0, 4)),
                   concat=bool(r.randint(0, 2)), cs=float(r.choice([1.0, 1e-5])) if prec == F16 else 1.0,
                   split=N, sorted=False, feat_bf16=False, pass_split=split, pass_tap=bool(r.randint(0, 2)),
                   p=float(RATES[r.randint(0, len(RATES))]))
        if route == "kv_source":
            cfg.update(Hi=int(r.randint(2, 20)), Wi=int(r.randint(2, 24)), feat_bf16=bool(r.randint(0, 2)))
            if not ops.kv_source_supported(cfg["C"], h, g, prec):
                continue
        return cfg
    raise AssertionError("no configuration drawn")


def _run(gpu, cfg, p, seed):
    kw = dict(heads=cfg["h"], groups=cfg["g"], views=cfg["V"], precision=cfg["prec"], concat_views=cfg["concat"],
              attn_drop=(p, seed))
    if cfg["pass_split"] is not None:
        kw["cell_split"] = cfg["pass_split"]
    if "feat" in gpu:
        return ops.attention_core(gpu["query"], None, None, gpu["pos"], gpu["table"],
                                  kv_source=(gpu["feat"], gpu["Wkv"], gpu["bkv"]), tap_source=cfg["pass_tap"], **kw)
    return ops.attention_core(gpu["query"], gpu["k"], gpu["v"], gpu["pos"], gpu["table"], **kw)


def _views_apart(out, cfg):
    """(B, M, V C) of concat_views -> (B V, M, C), the oracle's layout."""
    if not cfg["concat"]:
        return out
    B, V, C, M = cfg["B"], cfg["V"], cfg["C"], cfg["S"] ** 2
    assert out.shape == (B, M, V * C)
    return out.reshape(B, M, V, C).permute(0, 2, 1, 3).reshape(B * V, M, C)


@pytest.mark.parametrize("seed", list(range(NSEED)))
@pytest.mark.parametrize("route,prec", DROP_MODES, ids=[f"{r}-{MODE_NAME[p]}" for r, p in DROP_MODES])
def test_dropout_random_configuration(route, prec, seed):
    cfg = draw_drop(route, prec, seed)
    run_drop_case(cfg, 5000 + 97 * seed + prec)


def run_drop_case(cfg, seed):
    prec, p = cfg["prec"], cfg["p"]
    B, V, C, h, g, S, N = (cfg[k] for k in ("B", "V", "C", "h", "g", "S", "N"))
    Wt = 2 * S * cfg["D"] - 1
    ins = make(dict(cfg, route="kv_source" if cfg["route"] == "kv_source" else "kv_region"), seed)
    fused = "feat" in ins
    tag = f"{cfg}"
    dseed = 0x9e000000 + seed
    keep = drop_mult(dseed, p, B * V * h, S, N)

    # ---- float64 oracle ----
    cpu = {n: t.clone().double().requires_grad_(True) for n, t in ins.items()}
    k64, v64 = chain_kv(cpu["feat"], cpu["Wkv"], cpu["bkv"], cpu["pos"], g) if fused else (cpu["k"], cpu["v"])
    want = _oracle_core_drop(cpu["query"], k64, v64, cpu["pos"], cpu["table"], h, g, V, keep)     # (B V, M, C)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) * cfg["cs"]
    want.backward(cot)

    # ---- device, with the route recorded ----
    gpu = {n: t.clone().to(DEV).requires_grad_(True) for n, t in ins.items()}
    ops.KERNEL_TIMER.start()
    got = _views_apart(_run(gpu, cfg, p, dseed), cfg)
    got.backward(cot.float().to(DEV))
    used = set(ops.KERNEL_TIMER.stop())
    for k in DROP_KERNELS:
        assert k in used, f"{tag}: {k} did not run ({sorted(used)})"
    assert not set(OTHER_ATTN) & used, f"{tag}: {sorted(set(OTHER_ATTN) & used)} ran"
    if fused:
        assert "bevr_kv_project" in used, f"{tag}: {sorted(used)}"

    # ---- numbers ----
    e = rel_err(got.detach().cpu().double(), want.detach())
    assert e < OUT_LIM[prec], f"{tag}: out {e:.3e}"
    cs = cfg["cs"]
    clustered = cfg["kind"] == 2
    terms = None
    for n in ins:
        a, b = gpu[n].grad, cpu[n].grad
        assert a is not None and b is not None, f"{tag}: no gradient for {n}"
        a = a.cpu().double()
        assert torch.isfinite(a).all(), f"{tag}: grad {n} not finite"
        if n == "pos":
            clean = kink_distance(ins["pos"], S, Wt) >= 1e-4
            if fused:
                clean &= pixel_kink_distance(ins["pos"], ins["feat"].shape[1], ins["feat"].shape[2]) >= 1e-4
            assert clean.float().mean().item() > 0.5, f"{tag}: kink neighbourhood too wide for this case"
            dg, dw = a[clean], b[clean]
            ep = (dg - dw).norm().item() / max(dw.norm().item(), 2e-2 * cs * max(dw.numel(), 1) ** 0.5)
            assert ep < POS_LIM[prec], f"{tag}: grad pos 2-norm {ep:.3e}"
            continue
        scale = max(b.abs().max().item(), 2e-2 * cs)
        if n in ("table", "query") and clustered:
            # one tight cluster: the term bound of the routes sweep with D mask folded into the dP terms
            if terms is None:
                terms = gradient_terms([cpu["query"], k64, v64, cpu["pos"], cpu["table"]], cot, h, g, V, keep=keep)
            bound = 2.0 * UNIT[prec] * terms[n == "query"] + GRAD_LIM[prec] * scale
            worst = ((a - b).abs() / bound).max().item()
            assert worst < 1.0, f"{tag}: grad {n} {worst:.2f} x its term bound"
            continue
        e = (a - b).abs().max().item() / scale
        lim = GRAD_LIM[prec] + (2.0 ** -8 if n == "feat" and cfg["feat_bf16"] else 0.0)
        assert e < lim, f"{tag}: grad {n} {e:.3e}"

    # ---- the seed matters exactly where the mask does ----
    with torch.no_grad():
        nd = {n: t.detach() for n, t in gpu.items()}
        for s2 in range(dseed + 1, dseed + 65):
            same = torch.equal(drop_mult(s2, p, B * V * h, S, N), keep)
            if not same:
                break
        other = _views_apart(_run(nd, cfg, p, s2), cfg).cpu().double()
        base = got.detach().cpu().double()
        if same:
            # a handful of pairs at p of a few 2^-16: no seed nearby drops another pair -- nor may the output move
            assert rel_err(other, base) < 1e-6, f"{tag}: same mask, different output"
        else:
            assert rel_err(other, base) > 1e-6, f"{tag}: seed {s2} changed nothing"
