"""The error codes of every attention entry point that takes a descriptor, held against tests/golden/capi_error_codes.json
(tools/capi_error_table.py wrote it from the library as it was before the entry points' checks moved into one run() per
source file).  The cases are one defect and every pair of defects of different classes, so the table also pins the order
of the checks, which tests/test_capi_errors.py does not."""
import hashlib
import json
import os
import sys

import pytest
import torch

from bevrender_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import capi_error_table as gen  # noqa: E402

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="the accepted cases go on to a launch with made-up pointers: harmless with no device (the first runtime call "
           "fails), not something to do on a GPU that others share")

with open(gen.TABLE) as f:
    GOLDEN = json.load(f)


def test_the_table_covers_every_entry_point():
    assert GOLDEN["abi"] == _lib.ABI_VERSION
    assert sorted(GOLDEN["entry_points"]) == sorted(gen.entry_points(_lib.lib()))
    assert len(GOLDEN["entry_points"]) == 31


@pytest.mark.parametrize("name", sorted(GOLDEN["entry_points"]))
def test_codes_and_their_order(name):
    want = GOLDEN["entry_points"][name]
    cs = gen.cases(_lib.lib(), name)
    assert len(cs) == want["cases"] == len(want["codes"])
    assert hashlib.sha256("\n".join(n for n, _ in cs).encode()).hexdigest() == want["names_sha256"]
    got = "".join(call() for _, call in cs)
    wrong = [(n, w, g) for (n, _), w, g in zip(cs, want["codes"], got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(cs)} cases differ (case, recorded, now): {wrong[:8]}"
    assert got == want["codes"]
