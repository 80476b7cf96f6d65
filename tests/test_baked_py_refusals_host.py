"""CPU test of the refusals of the baked volumes' Python front-end, word for word: every call of tools/make_baked_py_refusals.py on
CPU tensors -- each single defect of the 26 public baked functions of ops, the five baked *_autograd functions and the util.bake
methods that refuse, a few pairs that pin the order of the checks, and the all-valid calls, which end in the "no CPU path" error that
names the first tensor looked at -- gives the exception type and the full message that the fixture recorded at the commit before the
front-end moved into ops_baked.py.  Nothing here needs a device."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest


def _tool(repo_root):
    spec = importlib.util.spec_from_file_location("make_baked_py_refusals", os.path.join(repo_root, "tools", "make_baked_py_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_refusal_of_the_baked_front_end_keeps_its_words(repo_root):
    tool = _tool(repo_root)
    want, _ = tool.unpack(json.load(open(tool.FIXTURE)))
    assert len(want) > 1200
    # the fixture itself: on the host nothing returns -- every call is refused, a valid one for having no CPU path
    assert all(kind in ("ValueError", "TypeError", "PixelNerfHipError") for kind, _ in want.values())
    assert sum("no CPU path" in message for _, message in want.values()) > 500
    got = tool.record("cpu")
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {label: (got[label], want[label]) for label in want if got[label] != want[label]}
    assert not wrong, wrong


def test_baked_march_is_the_named_function_it_must_pick(repo_root):
    """ops.baked_march against the named wrapper for every kind of stored tensor: the same outcome, and a refusal of `step` names
    the wrapper that spoke -- on the host too, where a valid call only gets as far as "no CPU path" """
    tool = _tool(repo_root)
    calls = tool.march_cases("cpu")
    assert len(calls) == 54
    for label, named, march in calls:
        want, got = tool.outcome(named), tool.outcome(march)
        assert got == want and want[0] != "", (label, got, want)
        if label.endswith("step=0.0"):
            assert want == ["ValueError", f"{label.split(' at ')[0]}: step must be finite and > 0, got 0.0"], (label, want)


@pytest.mark.parametrize("module", ["pixelnerf_amd.ops_baked", "pixelnerf_amd.ops"])
def test_either_front_end_module_imports_first(repo_root, module):
    """ops re-exports ops_baked and both stand on _ops_common: whichever a fresh interpreter imports first, there is no cycle"""
    done = subprocess.run([sys.executable, "-c", f"import {module}, sys; from pixelnerf_amd import ops, ops_baked; "
                           "assert ops.baked_render is ops_baked.baked_render and ops.baked_march is ops_baked.baked_march"],
                          cwd=repo_root, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
