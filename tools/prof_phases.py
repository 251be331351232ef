"""Phase clock breakdown (s_memtime stamps, csrc/bevr_prof.h) of one attention kernel on the SCA block of prof_sca.py:
    python tools/prof_phases.py <fwd|bwd_q|bwd_k|gather|slab|slab_x3>
Needs the instrumented build: make -C bevrender_amd/csrc PROF=1 OUTDIR=../lib_prof"""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# per kernel: counter slots, warm-up iterations (before the reset) and measured ones, the routing switches under which
# the SCA block runs that kernel at all (ops.gather_supported / slab_supported), and how its slots are printed
KERNELS = {
    "fwd": dict(slots=16, warm=0, iters=1, env={"BEVR_GATHER": "0"}, waves=(0, 7), per="n_step", counts=("n_step",),
                names=["region+consts", "frag+qk-mfma", "bias-loop", "softmax", "pv-mfma", "stage+barrier", "step-total", "n_step"]),
    "bwd_q": dict(slots=16, warm=0, iters=1, env={"BEVR_SLAB": "0"}, waves=(0, 7), per="n_step", counts=("n_region", "n_step"),
                  names=["region", "consts+frag+mfma", "r-loop", "stage+barrier", "end-barrier", "n_region", "dq-mfma", "n_step"]),
    "bwd_k": dict(slots=16, warm=0, iters=1, env={}, waves=(0, 11), per="n_it", counts=("n_it",),
                  names=["top(slide)", "frag+mfma", "taps+valu", "dv/dk mfma", "stage store", "barrier", "total", "n_it"]),
    "gather": dict(slots=32, warm=0, iters=2, env={}),
    "slab": dict(slots=48, warm=2, iters=1, env={}),
    # the split-bf16 slab kernel (csrc/attn_slab_bwd_q_x3.hip): the block in that mode, the switch on
    "slab_x3": dict(slots=48, warm=2, iters=1, env={"PREC": "bf16x3", "BEVR_TAP_X3": "1", "BEVR_SLAB_X3": "1"}),
}
GATHER_PRODUCER = ["", "advance+stage", "", "wait fills+kv", "barrier wait", "n", "issue fills", ""]
GATHER_ROWBLOCK = ["barrier wait", "compute", "wait fills", "", "loop total", "n", "", ""]


def report_waves(k, v):
    """two waves of 8 slots each: clocks per step, the counts as they are"""
    for w, wave in enumerate(k["waves"]):
        s = dict(zip(k["names"], v[8 * w: 8 * w + 8]))
        n = max(s[k["per"]], 1)
        print("wave", wave, {name: (x if name in k["counts"] else round(x / n, 1)) for name, x in s.items()})


def report_gather(v):
    for tag, names, o in (("producer", GATHER_PRODUCER, 0), ("wave 0", GATHER_ROWBLOCK, 8), ("wave 3", GATHER_ROWBLOCK, 16)):
        s = v[o:o + 8]
        n = max(s[5], 1)
        print(tag, {name: round(x / n, 1) for name, x in zip(names, s) if name and name != "n"}, "n", s[5])


def report_slab(v):
    for tag, b in (("worker wave 0", 0), ("worker wave 6", 16)):
        n = max(1, v[b + 3])
        print(f"{tag}: emissions {v[b+3]} (with a live key in half 0: {v[b+2]}), items {v[b+15]}; clk per emission: "
              f"barrier wait {v[b]/n:.0f}, emission body {v[b+1]/n:.0f} (key-row loop {v[b+4]/n:.0f}, dQ product {v[b+5]/n:.0f}); "
              f"per item: slab in {v[b+12]/max(1,v[b+15]):.0f}, slab out {v[b+13]/max(1,v[b+15]):.0f}")
    b = 32
    n = max(1, v[b + 3])
    print(f"producer: emissions {v[b+3]}; clk per emission: wait for loads {v[b]/n:.0f}, constants + stores {v[b+1]/n:.0f}, "
          f"barrier wait {v[b+2]/n:.0f}")


def main(tag):
    k = KERNELS[tag]
    for name, value in k["env"].items():
        os.environ.setdefault(name, value)
    import torch
    from bevrender_amd import _lib
    from prof_sca import run
    _lib.LIB_PATH = os.path.join(ROOT, "bevrender_amd", "lib_prof", "libbevrender_hip.so")
    if not os.path.exists(_lib.LIB_PATH):
        sys.exit(f"{_lib.LIB_PATH} not found: make -C bevrender_amd/csrc PROF=1 OUTDIR=../lib_prof")
    reader = getattr(_lib.lib(), "bevr_debug_prof_" + tag)
    buf = (C.c_ulonglong * k["slots"])()
    if k["warm"]:
        run(iters=k["warm"])
    reader(buf, 1)
    run(iters=k["iters"])
    torch.cuda.synchronize()
    reader(buf, 0)
    v = list(buf)
    {"gather": report_gather, "slab": report_slab, "slab_x3": report_slab}.get(tag, lambda v_: report_waves(k, v_))(v)


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in KERNELS:
        sys.exit(__doc__)
    main(sys.argv[1])
