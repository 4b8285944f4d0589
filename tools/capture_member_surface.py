#!/usr/bin/env python3
"""Records the public surface of the member trainers -- names, kinds and signatures, no code:

    python tools/capture_member_surface.py [--tree DIR] [--out out.json]

`DIR` goes in front of sys.path, so `rpo_amd` is that tree's Python.  Needs no GPU.  Run with the commit before the
members' shared bookkeeping moved to rpo_amd/members.py; tests/test_members_host.py holds every later tree to
tests/golden/member_trainers_surface.json for exact equality.

Per class (`RPOMulti`, `RPOSweep`, `LPSweep`, `CoCoOpMulti`, `CoOpSweep`, `MemberLoopMixin`): every public attribute that
`dir(cls)` reaches (its MRO included) with its kind -- function, property, staticmethod, classmethod or class attribute --
`str(inspect.signature(...))` of a callable (a property: of its getter) and the value of a plain constant.  Per module: the
public callables it defines (or re-exports from rpo_amd.members, where shared ones may live) and its public plain constants."""
import argparse
import importlib
import inspect
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("multi", "sweep", "lp_sweep", "coop_multi", "coop_sweep")
CLASSES = (("multi", "RPOMulti"), ("sweep", "RPOSweep"), ("lp_sweep", "LPSweep"), ("coop_multi", "CoCoOpMulti"),
           ("coop_sweep", "CoOpSweep"), ("multi", "MemberLoopMixin"))


def _plain(v):
    """(True, a JSON value) for a constant made of None / bool / int / float / str and tuples, lists or sets of them."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return True, v
    if isinstance(v, (tuple, list)):
        got = [_plain(x) for x in v]
        return all(ok for ok, _ in got), [x for _, x in got]
    if isinstance(v, (set, frozenset)):
        got = [_plain(x) for x in sorted(v)]
        return all(ok for ok, _ in got), [x for _, x in got]
    return False, None


def describe(static) -> dict:
    """One attribute as `inspect.getattr_static` finds it."""
    if isinstance(static, property):
        return {"kind": "property", "signature": str(inspect.signature(static.fget))}
    if isinstance(static, (staticmethod, classmethod)):
        return {"kind": type(static).__name__, "signature": str(inspect.signature(static.__func__))}
    if inspect.isfunction(static):
        return {"kind": "function", "signature": str(inspect.signature(static))}
    if inspect.isclass(static):
        return {"kind": "class", "signature": str(inspect.signature(static))}
    ok, value = _plain(static)
    return {"kind": "class attribute", "value": value} if ok else {"kind": "class attribute", "type": type(static).__name__}


def class_surface(cls) -> dict:
    return {name: describe(inspect.getattr_static(cls, name)) for name in dir(cls) if not name.startswith("_")}


def module_surface(mod) -> dict:
    out = {}
    for name, v in sorted(vars(mod).items()):
        if name.startswith("_") or inspect.ismodule(v):
            continue
        if inspect.isfunction(v) or inspect.isclass(v):
            if getattr(v, "__module__", None) in (mod.__name__, "rpo_amd.members"):
                out[name] = {"kind": "class" if inspect.isclass(v) else "function", "signature": str(inspect.signature(v))}
            continue
        ok, value = _plain(v)
        if ok:
            out[name] = {"kind": "constant", "value": value}
    return out


def surface() -> dict:
    mods = {m: importlib.import_module(f"rpo_amd.{m}") for m in MODULES}
    return {"classes": {c: class_surface(getattr(mods[m], c)) for m, c in CLASSES},
            "modules": {m: module_surface(mod) for m, mod in mods.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO, help="the tree whose rpo_amd is imported")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "member_trainers_surface.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import rpo_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(rpo_amd.__file__))) == os.path.abspath(args.tree)
    rec = surface()
    json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"{args.out}: " + ", ".join(f"{c} {len(v)}" for c, v in rec["classes"].items()))


if __name__ == "__main__":
    main()
