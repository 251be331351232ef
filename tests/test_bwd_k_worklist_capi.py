"""The work-list forms of the key-side backward entry points (bevr_attn_bwd_k_ws, bevr_attn_tap_bwd_k_ws and their
workspace queries: include/bevrender_hip.h) without a GPU: they exist with the header's prototypes, the workspace holds
one entry per unit plus the counter, a null workspace is refused before anything is launched, the ABI version is
unchanged, and the switch BEVR_BWDK_LIST is read per call."""
import ctypes as C

from bevrender_amd import _lib, ops
from test_capi_symbols import declared_prototypes

NEW = ("bevr_attn_bwd_k_ws", "bevr_attn_bwd_k_ws_bytes", "bevr_attn_tap_bwd_k_ws", "bevr_attn_tap_bwd_k_ws_bytes")


def desc(n_prob=48, heads=2, S=200, Wt=1999, N=35936, Np=35968, prec=_lib.PREC_BF16):
    d = _lib.AttnDesc()
    d.S, d.Wt = S, Wt
    assert _lib.lib().bevr_attn_table_dims(C.byref(d)) == 0
    d.n_prob, d.q_div, d.heads, d.groups, d.N, d.Np, d.precision = n_prob, 6, heads, 1, N, Np, prec
    return d


def test_new_symbols_match_the_header_and_the_abi_version_stays():
    L = _lib.lib()
    protos = declared_prototypes()
    old_k, old_t = protos["bevr_attn_bwd_k"], protos["bevr_attn_tap_bwd_k"]
    # the old argument lists with (workspace, max_workgroups) in front of the stream
    assert protos["bevr_attn_bwd_k_ws"] == ("int", old_k[1][:-1] + ["ptr", "int", "ptr"])
    assert protos["bevr_attn_tap_bwd_k_ws"] == ("int", old_t[1][:-1] + ["ptr", "int", "ptr"])
    for name in ("bevr_attn_bwd_k_ws_bytes", "bevr_attn_tap_bwd_k_ws_bytes"):
        assert protos[name] == ("size_t", ["desc"])
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.bevr_abi_version() == _lib.ABI_VERSION == 6


def test_workspaces_hold_one_entry_per_unit_and_the_counter():
    L = _lib.lib()
    d = desc()
    n_ph = d.n_prob * d.heads
    blocks = -(-d.Np // 384)                       # key blocks of the region kernels
    assert L.bevr_attn_bwd_k_ws_bytes(C.byref(d)) >= 4 * (n_ph * blocks + 1)
    t = desc(N=64064, Np=64064)
    tiles = t.Np // 32                             # 32-key tiles of the tap kernels
    got = L.bevr_attn_tap_bwd_k_ws_bytes(C.byref(t))
    assert got >= 4 * (n_ph * tiles + 1)
    assert got < 1 << 20                           # one entry per tile, not per (tile, column)
    bad = _lib.AttnDesc()
    assert L.bevr_attn_bwd_k_ws_bytes(C.byref(bad)) == 0 and L.bevr_attn_tap_bwd_k_ws_bytes(C.byref(bad)) == 0


def test_a_null_or_misaligned_workspace_is_refused_before_any_launch():
    L = _lib.lib()
    d = desc()
    one = C.c_void_p(16)                           # never dereferenced: the argument checks come first
    k_args = [C.byref(d)] + [one] * 16
    assert L.bevr_attn_bwd_k_ws(*k_args, None, 0, None) == -1
    assert L.bevr_attn_bwd_k_ws(*k_args, C.c_void_p(8), 0, None) == -4
    assert L.bevr_attn_bwd_k_ws(*k_args, one, -1, None) == -2
    assert L.bevr_attn_bwd_k_ws(C.byref(d), None, *[one] * 15, one, 0, None) == -1          # as the entry point without a list
    t_args = [C.byref(d)] + [one] * 8
    assert L.bevr_attn_tap_bwd_k_ws(*t_args, None, 0, None) == -1
    assert L.bevr_attn_tap_bwd_k_ws(*t_args, C.c_void_p(8), 0, None) == -4
    assert L.bevr_attn_tap_bwd_k_ws(*t_args, one, -1, None) == -2
    x3 = desc(prec=_lib.PREC_BF16X3)               # the split mode keeps the entry point without a list
    assert L.bevr_attn_tap_bwd_k_ws(C.byref(x3), *[one] * 8, one, 0, None) == -3


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("BEVR_BWDK_LIST", raising=False)
    assert ops.bwd_k_list()
    monkeypatch.setenv("BEVR_BWDK_LIST", "0")
    assert not ops.bwd_k_list()
    monkeypatch.setenv("BEVR_BWDK_LIST", "1")
    assert ops.bwd_k_list()
