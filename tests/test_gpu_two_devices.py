"""The per-device caches of csrc/attn_host.h (the CU count, a kernel's residency, its raised dynamic-LDS limit): ONE
process runs the kernels that use them on device 0 and then on device 1.  A cache that kept the first device's answer for
the process would leave device 1 with the 64 KB default of dynamic LDS (the slab and split-mode gather launches then
fail) or with device 0's grid size.

Nothing is restated here: under `with torch.cuda.device(i)` the tests of the three files are called as they stand --
their "cuda" is the current device -- so every device is held to the same references and limits as those tests hold
device 0 to: the slab backward in bf16 under BEVR_SLAB=2 (tests/test_gpu_slab.py, tsa_small), the split-mode gather
forward under BEVR_GATHER_X3=1 (tests/test_gpu_gather_x3.py, "31 / 32 / 33 keys": S = 5, the smallest case whose
gradients are compared) and the region key-side backward from the work list (tests/test_gpu_bwd_k_worklist.py; "middle":
S = 40 and 800 keys as every case of that file, and a list that is not empty).  A recorder around ops._launch checks
that the slab and gather entry points ran and that every launch happened with device i current."""
import pytest
import torch

import test_gpu_bwd_k_worklist as worklist
import test_gpu_gather_x3 as gather_x3
import test_gpu_slab as slab
from bevrender_amd import _lib, ops

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")]


def on_device(i, monkeypatch):
    """the three problems with device i current; every launch through ops._launch is seen"""
    seen = []
    launch = ops._launch

    def recording(entry, *a, **kw):
        seen.append((entry, torch.cuda.current_device()))
        return launch(entry, *a, **kw)
    name, cfg, pos_fn = gather_x3.CASES[-1]
    with monkeypatch.context() as m, torch.cuda.device(i):
        m.setattr(ops, "_launch", recording)
        assert torch.zeros(1, device=slab.DEV).device.index == i
        slab.test_slab_bwd_q_agrees_with_the_query_tile_kernel("tsa_small", _lib.PREC_BF16)
        gather_x3.test_cases_against_the_oracle_and_the_region_forward(name, cfg, pos_fn, monkeypatch)
        worklist.region_case("middle", _lib.PREC_BF16, m)      # its hook on the key-side backward ends with the context
        torch.cuda.synchronize()
    ran = {e for e, _ in seen}
    assert {"bevr_attn_slab_bwd_q", "bevr_attn_gather_fwd_x3"} <= ran, (i, sorted(ran))
    assert all(dev == i for _, dev in seen), (i, seen)


def test_slab_gather_x3_and_work_list_on_device_0_then_1(monkeypatch):
    for i in (0, 1):
        on_device(i, monkeypatch)
