"""The member trainers after their shared bookkeeping moved to rpo_amd/members.py: the public surface is the one recorded
before the move (tests/golden/member_trainers_surface.json, tools/capture_member_surface.py), and what is shared is ONE
function object on every trainer that has it.  No GPU."""
import importlib.util
import inspect
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the move itself adds to a recorded surface, and nothing else: the member-major step is stated on `MemberLoopMixin`
# (it was written out on RPOMulti and on CoCoOpMulti), and CoCoOpMulti's per-member `model-best` bookkeeping, which its
# `train` held inline, is the `after_epoch_eval` of the two sweeps.  Both are held to the signature recorded for the
# trainer that had them.
MOVED_IN = {("MemberLoopMixin", "step_async"): ("RPOMulti", "step_async"),
            ("CoCoOpMulti", "after_epoch_eval"): ("CoOpSweep", "after_epoch_eval")}


def _capture():
    spec = importlib.util.spec_from_file_location("capture_member_surface",
                                                  os.path.join(REPO, "tools", "capture_member_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_public_surface_is_the_recorded_one():
    want = json.load(open(os.path.join(REPO, "tests", "golden", "member_trainers_surface.json")))
    got = json.loads(json.dumps(_capture().surface()))                       # (tuples -> lists, as the file holds them)
    for (cls, name), (src_cls, src_name) in MOVED_IN.items():
        assert name not in want["classes"][cls], f"{cls}.{name} was there before: take it out of MOVED_IN"
        assert got["classes"][cls].pop(name) == want["classes"][src_cls][src_name], f"{cls}.{name}"
    assert sorted(got["modules"]) == sorted(want["modules"]) and sorted(got["classes"]) == sorted(want["classes"])
    for kind in ("classes", "modules"):
        for owner in want[kind]:
            w, g = want[kind][owner], got[kind][owner]
            assert sorted(g) == sorted(w), f"{owner}: missing {sorted(set(w) - set(g))}, added {sorted(set(g) - set(w))}"
            for name in w:
                assert g[name] == w[name], f"{owner}.{name}: {g[name]} != recorded {w[name]}"
    assert got == want


def _trainers():
    from rpo_amd.coop import CoCoOp, CoOp
    from rpo_amd.coop_multi import CoCoOpMulti
    from rpo_amd.coop_sweep import CoOpSweep
    from rpo_amd.lp import LP
    from rpo_amd.lp_sweep import LPSweep
    from rpo_amd.multi import RPOMulti
    from rpo_amd.sweep import RPOSweep
    return dict(RPOMulti=RPOMulti, RPOSweep=RPOSweep, LPSweep=LPSweep, CoCoOpMulti=CoCoOpMulti, CoOpSweep=CoOpSweep,
                CoOp=CoOp, CoCoOp=CoCoOp, LP=LP)


ONE_DEFINITION = [("update_lr", ("RPOSweep", "LPSweep", "CoCoOpMulti", "CoOpSweep")),
                  ("_check_member", ("RPOMulti", "RPOSweep", "LPSweep", "CoCoOpMulti", "CoOpSweep")),
                  ("step_async", ("RPOMulti", "RPOSweep", "CoCoOpMulti")),
                  ("after_epoch_eval", ("LPSweep", "CoOpSweep", "CoCoOpMulti")),
                  ("save_model", ("LPSweep", "CoCoOpMulti", "CoOpSweep")),
                  ("_save_member", ("LPSweep", "CoCoOpMulti", "CoOpSweep")),
                  ("parse_batch_train", ("CoOp", "CoCoOp", "LP", "LPSweep", "CoOpSweep"))]


@pytest.mark.parametrize("name,owners", ONE_DEFINITION, ids=[n for n, _ in ONE_DEFINITION])
def test_shared_methods_are_one_function_object(name, owners):
    classes = _trainers()
    fns = [inspect.getattr_static(classes[c], name) for c in owners]
    assert all(inspect.isfunction(f) for f in fns), f"{name}: {[type(f).__name__ for f in fns]}"
    assert all(f is fns[0] for f in fns), f"{name} is defined {len({id(f) for f in fns})} times on {owners}"


def test_skipped_steps_is_one_body_behind_a_method_and_a_property():
    """The body is one function; CoCoOpMulti exposes it as a property, the other three as a method (recorded as known in
    DESIGN.md section 9t; the surface test pins both forms)."""
    classes = _trainers()
    body = inspect.getattr_static(classes["RPOSweep"], "skipped_steps")
    assert inspect.isfunction(body)
    assert all(inspect.getattr_static(classes[c], "skipped_steps") is body for c in ("LPSweep", "CoOpSweep"))
    prop = inspect.getattr_static(classes["CoCoOpMulti"], "skipped_steps")
    assert isinstance(prop, property) and prop.fget is body


def test_multi_still_exports_what_moved():
    from rpo_amd import members, multi
    for name in ("MemberLoopMixin", "member_batches", "seeded_prompts", "member_checkpoint", "read_member_checkpoint"):
        assert getattr(multi, name) is getattr(members, name)
    assert inspect.signature(multi.member_batches).parameters["who"].default == "RPOMulti"
