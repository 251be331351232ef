"""The phase-stamp build of the library (make PROF=1, csrc/bevr_prof.h) links, exports one counter reader per
instrumented kernel beside the whole C ABI, and the shipped library carries none of them.  Nothing is launched (no GPU
needed); the variant translation units (dropout, split-bf16, row bands) include the instrumented sources a second
time, which is what once made this build fail with duplicate symbols."""
import ctypes
import os
import subprocess

from bevrender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF_LIB = os.path.join(ROOT, "bevrender_amd", "lib_prof", "libbevrender_hip.so")
READERS = ["bevr_debug_prof_" + tag for tag in ("fwd", "bwd_q", "bwd_k", "gather", "slab")]


def test_instrumented_build_links_and_exports_the_readers():
    if not os.path.exists(PROF_LIB):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "bevrender_amd", "csrc"), "-j", "4", "PROF=1",
                            "OUTDIR=../lib_prof"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    L = ctypes.CDLL(PROF_LIB)
    for name in READERS + _lib.SYMBOLS:
        assert hasattr(L, name), name


def test_shipped_library_has_no_readers():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in READERS:
        assert not hasattr(L, name), name
