"""The error contract of the attention entry points, as a table: tests/golden/capi_error_codes.json (and, for entry
points added after it was recorded, a table per group beside it: LATER).

`python tools/capi_error_table.py` calls every attention entry point that takes a descriptor with one defect and with
every pair of defects of different classes, and records the code each call returns.  The pairs pin the ORDER of the
checks: which of two violated clauses an entry point reports.  tests/test_capi_error_table.py builds the same cases and
holds the built library against the committed table, character by character.

Run it WITHOUT a GPU: the checks come before any launch, so a rejected call touches nothing, but an accepted one goes
on to a launch with made-up pointers.  With no device the first runtime call of that launch returns hipErrorNoDevice
(a positive code, recorded as "accepted"); on a device it would be a launch on memory nobody owns.

A call is built from the binding's argtypes alone (bevrender_amd/_lib.py): pointers are 0x10000 and the last one, the
stream, is NULL; the int arguments are (row0, n_rows) = (0, S) where there are two and max_workgroups = 0 where there is
one; the unsigned ones are (thr, seed) = (100, 1), preceded by key0 = 0 where there are three.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevrender_amd import _lib, ops  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                     "capi_error_codes.json")
CODES = {-1: "N", -2: "S", -3: "P", -4: "A"}      # BEVR_E_NULL, _SHAPE, _PRECISION, _ALIGN; "." = accepted (>= 0)
GOOD, ODD = 0x10000, 0x10004                       # a 16-byte aligned, never dereferenced "device pointer"; a misaligned one
BASE = dict(n_prob=2, q_div=1, heads=2, groups=1, S=12, N=100, Wt=71)     # the descriptor of tests/test_capi_errors.py
BAD_DESCS = [dict(Sp=16), dict(Np=101), dict(Ht=20), dict(heads=3, groups=2), dict(n_prob=3, q_div=2), dict(Hp=7)]
# the size limits tests/test_capi_errors.py uses: a descriptor that is valid, and too large for that entry point
SIZE_LIMITS = {
    "bevr_attn_cell_fwd": dict(n_prob=1, q_div=1, heads=1, groups=1, S=530, N=64, Wt=2 * 530 - 1),
    "bevr_attn_gather_fwd": dict(n_prob=1, q_div=1, heads=1, groups=1, S=230, N=64, Wt=2 * 230 - 1),
}


# Entry points added AFTER capi_error_codes.json was recorded.  That table is a record of the library at one point and stays
# what it is; a later group's rows -- the same cases, built by the same functions -- go into a table of its own, beside the
# test file that came with the group: {group: (table file under tests/golden, its entry points)}.
LATER = {
    "scatter_dropout": ("scatter_dropout_error_codes.json",
                        ("bevr_attn_gather_fwd_dropout", "bevr_attn_slab_drop_prep", "bevr_attn_slab_bwd_q_dropout")),
    "slab_x3_dropout": ("slab_x3_dropout_error_codes.json",
                        ("bevr_attn_slab_x3_drop_prep", "bevr_attn_slab_bwd_q_x3_dropout")),
    "tap_groups": ("tap_groups_error_codes.json",
                   ("bevr_attn_tap_g2_prep", "bevr_attn_tap_g2_fwd", "bevr_attn_tap_g2_bwd_q", "bevr_attn_tap_g2_bwd_k")),
    "slab_x3_rows": ("slab_x3_rows_error_codes.json", ("bevr_attn_slab_x3_rows_prep", "bevr_attn_slab_bwd_q_x3_rows")),
}
# descriptor fields a group's entry points need on top of BASE to accept a call (the tap entry points for two channel
# groups take groups == 2 only; their "groups" defect, heads=2,groups=2, is then no defect and is recorded as accepted)
LATER_BASE = {"tap_groups": dict(groups=2)}


def base_of(name):
    """BASE as the entry point's group needs it"""
    for group, (_, names) in LATER.items():
        if name in names:
            return dict(BASE, **LATER_BASE.get(group, {}))
    return dict(BASE)


def later_table(group):
    return os.path.join(os.path.dirname(TABLE), LATER[group][0])


def entry_points(L, group=None):
    """Every bevr_attn_* symbol whose first argument is the descriptor and whose result is an int code: those of the
    recorded table (group None: all but the LATER groups), or those of one LATER group."""
    dp = C.POINTER(_lib.AttnDesc)
    later = {n for _, names in LATER.values() for n in names}
    out = []
    for name in _lib.SYMBOLS:
        fn = getattr(L, name)
        if (name.startswith("bevr_attn_") and name != "bevr_attn_table_dims" and fn.restype is C.c_int
                and fn.argtypes and fn.argtypes[0] is dp):
            if (name in LATER[group][1]) if group else (name not in later):
                out.append(name)
    return out


class Call:
    """One call of an entry point: a geometry, descriptor fields set afterwards, and per-argument overrides."""

    def __init__(self, L, name, precision):
        self.fn, self.name = getattr(L, name), name
        self.geom = dict(base_of(name), precision=precision)
        self.fields, self.args, self.no_desc = {}, {}, False
        types = self.fn.argtypes
        self.pointers = [i for i, t in enumerate(types) if i and t is C.c_void_p][:-1]     # the last one is the stream
        self.ints = [i for i, t in enumerate(types) if t is C.c_int]
        self.uints = [i for i, t in enumerate(types) if t is C.c_uint32]
        assert len(self.ints) in (0, 1, 2) and len(self.uints) in (0, 2, 3), name
        assert len(self.pointers) + len(self.ints) + len(self.uints) + 2 == len(types), name

    def __call__(self):
        d = ops.AttnGeom(**self.geom).desc()
        for k, v in self.fields.items():
            setattr(d, k, v)
        types = self.fn.argtypes
        a = [None if self.no_desc else C.byref(d)] + [None] * (len(types) - 1)
        for i in self.pointers:
            a[i] = GOOD
        if len(self.ints) == 2:
            a[self.ints[0]], a[self.ints[1]] = 0, d.S                       # row0, n_rows
        elif self.ints:
            a[self.ints[0]] = 0                                             # max_workgroups
        for i, v in zip(self.uints, (0, 100, 1) if len(self.uints) == 3 else (100, 1)):   # [key0,] thr, seed
            a[i] = v
        for i, v in self.args.items():
            a[i] = v(d) if callable(v) else v
        rc = self.fn(*a)
        return "." if rc >= 0 else CODES.get(rc, "?")


def first_precision(L, name):
    for prec in (_lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_BF16X3):
        if Call(L, name, prec)() == ".":
            return prec
    raise AssertionError(f"{name} accepts no precision with valid arguments")


def defects(call):
    """(class, name, apply) of every single defect of this entry point, in a fixed order.  Two defects of one class are
    never paired: they are alternatives (two values of one field)."""
    out = []

    def add(cls, name, fn):
        out.append((cls, name, fn))

    add("null:0", "null:0", lambda c: setattr(c, "no_desc", True))
    for i in call.pointers:
        add(f"null:{i}", f"null:{i}", lambda c, i=i: c.args.__setitem__(i, None))
    for i in call.pointers:
        add(f"odd:{i}", f"odd:{i}", lambda c, i=i: c.args.__setitem__(i, ODD))
    for p in (0, 1, 2, 3, 9):
        add("precision", f"precision={p}", lambda c, p=p: c.fields.__setitem__("precision", p))
    add("groups", "heads=2,groups=2", lambda c: c.fields.update(heads=2, groups=2))
    for bad in BAD_DESCS:
        add("descriptor", "desc:" + ",".join(f"{k}={v}" for k, v in bad.items()), lambda c, bad=bad: c.fields.update(bad))
    if call.name in SIZE_LIMITS:
        big = SIZE_LIMITS[call.name]
        add("descriptor", f"desc:S={big['S']}", lambda c, big=big: c.geom.update(big))
    if call.uints:
        thr = call.uints[-2]
        add("scalar", "thr=65536", lambda c: c.args.__setitem__(thr, 65536))
    if len(call.ints) == 2:
        row0, n_rows = call.ints
        add("scalar", "row0=1", lambda c: c.args.__setitem__(row0, 1))
        add("scalar", "n_rows=0", lambda c: c.args.__setitem__(n_rows, 0))
        add("scalar", "n_rows=S+1", lambda c: c.args.__setitem__(n_rows, lambda d: d.S + 1))
    elif call.ints:
        add("scalar", "max_workgroups=-1", lambda c: c.args.__setitem__(call.ints[0], -1))
    return out


def cases(L, name):
    """[(case name, Call)] of one entry point: no defect, every single defect, every pair of different classes."""
    prec = first_precision(L, name)
    single = defects(Call(L, name, prec))
    combos = [()] + [(s,) for s in single] + [p for p in itertools.combinations(single, 2) if p[0][0] != p[1][0]]
    out = []
    for combo in combos:
        call = Call(L, name, prec)
        for _, _, apply in combo:
            apply(call)
        out.append(("+".join(n for _, n, _ in combo) or "valid", call))
    return out


def table(L, group=None):
    entries = {}
    for name in entry_points(L, group):
        cs = cases(L, name)
        entries[name] = {
            "cases": len(cs),
            "names_sha256": hashlib.sha256("\n".join(n for n, _ in cs).encode()).hexdigest(),
            "codes": "".join(call() for _, call in cs),
        }
    return {"abi": _lib.ABI_VERSION, "legend": "N S P A = BEVR_E_NULL _SHAPE _PRECISION _ALIGN, . = accepted",
            "entry_points": entries}


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("run this without a GPU: the accepted cases reach a launch with made-up pointers")
    for group, path in [(None, TABLE)] + [(g, later_table(g)) for g in LATER]:
        t = table(_lib.lib(), group)
        with open(path, "w") as f:
            json.dump(t, f, indent=1)
            f.write("\n")
        n = sum(e["cases"] for e in t["entry_points"].values())
        print(f"{len(t['entry_points'])} entry points, {n} cases -> {path}")


if __name__ == "__main__":
    main()
