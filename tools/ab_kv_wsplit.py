"""Launch time of bevr_kv_project_w2 (split hi + lo weights) against bevr_kv_project at the benchmark's SCA shape.

One launch = the scattered key segment of an SCA call of the benchmark: 48 problems (B = 8 x 6 views), 64 x 176 feature
map with 64 channels (bf16, as the benchmark stages it), 2 heads, N = 36 000 keys per problem, with the transposed K and
both norm outputs (a training step's call).  Both entry points on the same inputs, alternating in ONE process, HIP
events around every launch, 3 warm-up rounds, then ROUNDS (default 9, at least 5) timed rounds; min and median per entry
point, in bf16 (lo_exp = 0: one sweep with a second MFMA) and fp16 (lo_exp = 11: a sweep per plane).

    python tools/ab_kv_wsplit.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevrender_amd import _lib, ops  # noqa: E402

DEV = "cuda"
ROUNDS = max(5, int(os.environ.get("ROUNDS", "9")))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def main():
    nb, Hi, Wi, Cc, h, N = 48, 64, 176, 64, 2, 36000
    Np = 64 * ((N + 63) // 64)
    L = _lib.lib()
    gen = torch.Generator().manual_seed(3)
    feat = torch.rand(nb, Hi, Wi, Cc, generator=gen).to(torch.bfloat16).to(DEV)
    pos = (torch.rand(nb, N, 2, generator=gen) * 2.0 - 1.0).to(DEV)
    W = (torch.randn(2 * Cc, Cc, generator=gen) / Cc ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(2 * Cc, generator=gen)).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"what": "one launch: %d problems, %d x %d x %d bf16 map, %d heads, N = %d keys, Kt and both norms; HIP events, "
                   "entry points alternating, %d rounds after 3 warm-up rounds" % (nb, Hi, Wi, Cc, h, N, ROUNDS)}
    for tag, prec in (("bf16", _lib.PREC_BF16), ("f16", _lib.PREC_F16)):
        ed = ops._edtype(prec)
        Kr = torch.empty(nb, h, Np, 32, device=DEV, dtype=ed)
        Vr, Kt, Vt = torch.empty_like(Kr), torch.empty(nb, h, 32, Np, device=DEV, dtype=ed), torch.empty(nb, h, 32, Np, device=DEV, dtype=ed)
        vn2, kn2 = torch.zeros(1, device=DEV), torch.zeros(nb, h, device=DEV)
        We = W.to(ed).contiguous()
        W2, lo_exp = ops.kv_split_weights(W, prec)
        tail = (ptr(bias), nb, Hi, Wi, Cc, N, Np, h, Cc // h, prec, ptr(Kr), ptr(Vr), ptr(Kt), ptr(Vt), ptr(vn2), ptr(kn2), 1, st)
        head = (ptr(feat), 1, ptr(pos), N)
        calls = {"bevr_kv_project": lambda: L.bevr_kv_project(*head, ptr(We), *tail),
                 "bevr_kv_project_w2": lambda: L.bevr_kv_project_w2(*head, ptr(W2), lo_exp, *tail)}
        ms = {k: [] for k in calls}
        for it in range(ROUNDS + 3):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = call()
                e1.record()
                torch.cuda.synchronize()
                _lib.check(rc, name)
                if it >= 3:
                    ms[name].append(e0.elapsed_time(e1))
        row = {k: {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4)}
               for k, v in ms.items()}
        row["lo_exp"] = lo_exp
        row["w2_over_plain_median"] = round(row["bevr_kv_project_w2"]["median_ms"] / row["bevr_kv_project"]["median_ms"], 3)
        row["w2_over_plain_min"] = round(row["bevr_kv_project_w2"]["min_ms"] / row["bevr_kv_project"]["min_ms"], 3)
        res[tag] = row
    print(json.dumps(res, indent=1))
    if sys.argv[1:]:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
