"""GPU test of the refusals of the baked volumes' Python front-end that lie BEHIND its first device check, word for word: the calls
of tools/make_baked_py_refusals.py that need no object of util.bake, on HIP tensors without a single ray -- the shapes and dtypes of
d_rgb, d_depth and d_alpha, `out` of the wrong shape or not contiguous, the `want` and `out` lists, a shared buffer given twice,
misaligned storage, `scale` -- give the exception type and the full message, or return the shapes, that the fixture recorded on an
MI355X at the commit before the front-end moved into ops_baked.py.  No call launches a kernel: it is refused, or it has R = 0."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _tool(repo_root):
    spec = importlib.util.spec_from_file_location("make_baked_py_refusals", os.path.join(repo_root, "tools", "make_baked_py_refusals.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_every_refusal_behind_the_first_device_check_keeps_its_words(repo_root):
    tool = _tool(repo_root)
    fixture = json.load(open(tool.FIXTURE))
    host, want = tool.unpack(fixture)  # the device's outcome of a label: the host's, unless the fixture's device section says another
    assert len(want) > 1000 and sum(len(d) for d in fixture["device"].values()) > 400 and sum(kind == "" for kind, _ in want.values()) > 100  # (no rays: it returned)
    got = tool.record("cuda:0")
    if torch.cuda.device_count() >= 2 > fixture["device_count"]:  # the fixture saw one device: the two-device calls have no record
        got = {label: g for label, g in got.items() if "two devices" not in label}
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {label: (got[label], want[label]) for label in want if got[label] != want[label]}
    assert not wrong, wrong


def test_baked_march_is_the_named_function_it_must_pick(repo_root):
    """ops.baked_march against the named wrapper for every kind of stored tensor, without a ray: a valid call returns the same
    shapes, and a refusal behind the first device check (`bits` of the wrong size) names the wrapper that spoke"""
    tool = _tool(repo_root)
    calls = tool.march_cases("cuda:0")
    assert len(calls) == 54
    for label, named, march in calls:
        want, got = tool.outcome(named), tool.outcome(march)
        assert got == want, (label, got, want)
        function = label.split(" at ")[0]
        if label.endswith("valid"):
            assert want == ["", "returned [(0, 3), (0,), (0,)]"], (label, want)
        elif label.endswith("bits of 2"):
            assert want == ["ValueError", f"{function}: bits must be the (1,) int32 tensor of occupancy_build for reso (2, 2, 2)"], (label, want)
