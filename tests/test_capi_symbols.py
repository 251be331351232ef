"""The C-ABI library loads and exports every symbol include/bevrender_hip.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

from bevrender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bevr_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_list_agree():
    assert declared_symbols() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(L, name), name
    L.bevr_abi_version.restype = ctypes.c_int
    assert L.bevr_abi_version() == _lib.ABI_VERSION == 6


def declared_prototypes():
    """{name: (return kind, [argument kinds])} of every prototype in the header.

    Grammar: `int|size_t|const char* name(args);`.  An argument is a descriptor pointer ("desc"), any other pointer
    ("ptr"), or a scalar "int", "longlong", "float", "u32" (`unsigned` / `uint32_t`), "size_t"."""
    src = open(os.path.join(ROOT, "include", "bevrender_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    scalars = {"int": "int", "int32_t": "int", "long long": "longlong", "float": "float", "unsigned": "u32",
               "unsigned int": "u32", "uint32_t": "u32", "size_t": "size_t"}
    protos = {}
    for ret, name, args in re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(bevr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        kinds = []
        args = " ".join(args.split())
        for arg in ([] if args in ("", "void") else args.split(",")):
            arg = arg.strip()
            if "*" in arg:
                kinds.append("desc" if re.search(r"\bbevr_attn_desc\b", arg) else "ptr")
                continue
            m = re.fullmatch(r"(?:const )?(.+?) ([A-Za-z_][A-Za-z0-9_]*)", arg)
            assert m and m.group(1) in scalars, (name, arg)
            kinds.append(scalars[m.group(1)])
        assert name not in protos, name
        protos[name] = ("cstr" if "char" in ret else ret, kinds)
    return protos


def binding_kind(t):
    if t is ctypes.POINTER(_lib.AttnDesc):
        return "desc"
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    # ctypes aliases types of equal size (c_uint32 is c_uint, c_size_t is c_ulong, ...): compare by identity in an order
    # that keeps the C ABI's distinctions (width, signedness, float) and nothing else
    for kind, ct in (("int", ctypes.c_int), ("longlong", ctypes.c_longlong), ("float", ctypes.c_float),
                     ("u32", ctypes.c_uint32), ("size_t", ctypes.c_size_t), ("cstr", ctypes.c_char_p)):
        if t is ct:
            return kind
    return repr(t)


def test_header_and_binding_agree_on_every_prototype():
    """Argument by argument and return type by return type: a swapped int / long long or a missing argument in a
    hand-written argtypes list would load and run."""
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(_lib.SYMBOLS)
    L = _lib.lib()
    bad = {}
    for name, (ret, kinds) in sorted(protos.items()):
        fn = getattr(L, name)
        have = (binding_kind(fn.restype), [binding_kind(t) for t in (fn.argtypes or [])])
        if have != (ret, kinds):
            bad[name] = {"header": (ret, kinds), "binding": have}
    assert not bad, bad


def test_argument_contract_is_checked_without_a_gpu():
    """Bad descriptors / NULL pointers are rejected before anything is launched."""
    L = _lib.lib()
    d = _lib.AttnDesc()
    assert L.bevr_attn_table_dims(ctypes.byref(d)) == -2            # S < 2
    d.S, d.Wt = 200, 1999
    assert L.bevr_attn_table_dims(ctypes.byref(d)) == 0
    assert (d.Sp, d.Ht, d.Hp, d.y_off, d.x_off, d.Wp) == (224, 399, 851, 226, 1003, 4006)
    d.n_prob, d.q_div, d.heads, d.groups, d.N, d.Np, d.precision = 24, 6, 2, 1, 100000, 100032, 1
    assert L.bevr_attn_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None) == -1
    d.Np = 100000                                                    # not a multiple of 64
    assert L.bevr_attn_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None) == -2
    assert L.bevr_sample_fwd(None, None, None, 1, 4, 4, 8, 4, None) == -1
    d.Np = 100032
    assert L.bevr_attn_key_ws_bytes(ctypes.byref(d)) == 24 * 100032 * 16 + 24 * (100032 // 32) * 16 * (1 + 8)
    assert L.bevr_attn_key_prep(ctypes.byref(d), None, None, None, None) == -1
    assert L.bevr_dwconv_fwd(None, None, None, None, 1, 4, 4, 8, 3, 1, 0, None) == -1
    one = ctypes.c_void_p(16)                                        # never dereferenced: the shape check comes first
    assert L.bevr_dwconv_fwd(one, one, None, one, 1, 4, 4, 8, 4, 1, 0, None) == -2     # even kernel size
    assert L.bevr_dwconv_bwd_w(one, one, one, None, 1, 4, 4, 8, 7, 0, None) == -2       # k > 5
    assert b"contract" in L.bevr_strerror(-2)


def test_ops_refuse_cpu_tensors():
    import torch
    from bevrender_amd import ops
    with pytest.raises(_lib.BevrError):
        ops.sample_features(torch.zeros(1, 4, 4, 4), torch.zeros(1, 3, 2), 1)
